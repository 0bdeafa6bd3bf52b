"""The host-pointer entry points at the edges of their staging: empty batches, arrays of no
bytes, optional arguments absent and given, and a scratch buffer that has to grow between two
calls.  Every host form stages its arrays through one helper (csrc/host_staging.h) whose one
rule is that a copy is skipped when it has no bytes or no host pointer; a copy that rule drops
or a device pointer it nulls shows here as a result that differs from the oracle's or from the
_device form's on the same arrays.

Small snapshots on purpose: TAS 130 nodes (three bitmap words, the last one partial) x 3
metrics, GAS 5 nodes x 3 cards x 2 resources.

Pinned elsewhere too, at other shapes: rows wider than the longest request keep the caller's
words (test_request_batch.py::test_filter_batch_matches_oracle_gathered_to_positions), a
placement of no pods (test_gas_place.py::test_place_no_pods), a node update of no updates
(test_gas_nodes.py::test_update_matches_the_replay_and_the_oracle[0-...]).  They are repeated
here on the small snapshots because this file also holds them against the _device forms."""
import ctypes
import itertools

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from helpers import unpack_bits, w64
from oracle import RULE_DTYPE
from test_gas_place import place_oracle
from test_request_batch import check_rows, gather_bits

pytestmark = pytest.mark.gpu

N, M = 130, 3
W = w64(N)
GN, GK, GQ = 5, 3, 2
FILTER, PRIORITIZE = _lib.PAS_TAS_FILTER, _lib.PAS_TAS_PRIORITIZE
SENTINEL = np.uint64(0xC3C3C3C3C3C3C3C3)
_gen = [91_000]


def dev(a):
    """A numpy array on the device (unsigned and record types as same-sized signed ints)."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == RULE_DTYPE:
        a = a.view(np.int64)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def filled(shape, dtype):
    import torch
    return torch.full(shape, 77, dtype=dtype, device="cuda")


def stream():
    import torch
    return torch.cuda.current_stream()


def sync():
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------- TAS

def tas_values():
    rng = np.random.default_rng(0xED6E)
    v = rng.integers(0, 5, (M, N)).astype(np.int64) * 1000
    pres_b = rng.random((M, N)) >= 0.2
    pres = np.zeros((M, W), np.uint64)
    for m, n in zip(*np.nonzero(pres_b)):
        pres[m, n >> 6] |= np.uint64(1) << np.uint64(n & 63)
    return v, pres


V, PRES = tas_values()


def set_tas(c):
    _gen[0] += 10
    c.tas_snapshot_set(_gen[0], V, PRES)
    return _gen[0]


def make_pods(p, rules_per_pod, seed=1):
    rng = np.random.default_rng(seed)
    rules = np.zeros(p * rules_per_pod, RULE_DTYPE)
    rules["metric"] = rng.integers(0, M, len(rules))
    rules["op"] = rng.integers(0, 3, len(rules))
    rules["target"] = rng.integers(0, 5, len(rules))
    rule_off = (np.arange(p + 1) * rules_per_pod).astype(np.int32)
    prio = np.zeros(p, RULE_DTYPE)
    prio["metric"] = rng.integers(0, M, p)
    prio["op"] = rng.integers(0, 3, p)
    cand = rng.integers(0, 2**63, (p, W), dtype=np.int64).astype(np.uint64)
    cand[:, W - 1] &= np.uint64((1 << (N - 64 * (W - 1))) - 1)
    return rules, rule_off, prio, cand


def eval_device(c, gen, rules, rule_off, prio, cand, flags):
    import torch
    p = len(rule_off) - 1
    pass_t = filled((p, W), torch.int64) if flags & FILTER else None
    order_t = filled((p, N), torch.int32) if flags & PRIORITIZE else None
    len_t = filled((p,), torch.int32) if flags & PRIORITIZE else None
    c.tas_eval_device(gen, p, len(rules), dev(rules), dev(rule_off), dev(prio),
                      None if cand is None else dev(cand), flags, pass_t, order_t, len_t,
                      stream=stream())
    sync()
    return (None if pass_t is None else pass_t.cpu().numpy().view(np.uint64),
            None if order_t is None else order_t.cpu().numpy(),
            None if len_t is None else len_t.cpu().numpy())


def assert_eval(got, want, flags, what):
    gp, go, gl = got
    wp, wo, wl_ = want
    if flags & FILTER:
        np.testing.assert_array_equal(gp, wp, err_msg=what + ": pass")
    else:
        assert gp is None
    if flags & PRIORITIZE:
        np.testing.assert_array_equal(gl, wl_, err_msg=what + ": lengths")
        for p in range(len(wl_)):
            np.testing.assert_array_equal(go[p, :gl[p]], wo[p, :wl_[p]],
                                          err_msg=f"{what}: order of pod {p}")
    else:
        assert go is None and gl is None


@pytest.mark.parametrize("flags", [FILTER, PRIORITIZE, FILTER | PRIORITIZE])
@pytest.mark.parametrize("with_cand", [False, True])
@pytest.mark.parametrize("pods,rules_per_pod", [(0, 0), (3, 0), (3, 2)])
def test_tas_eval(ctx, oracle, pods, rules_per_pod, with_cand, flags):
    gen = set_tas(ctx)
    rules, rule_off, prio, cand = make_pods(pods, rules_per_pod)
    cand = cand if with_cand else None
    assert len(rules) == pods * rules_per_pod and (rule_off == 0).all() == (len(rules) == 0)
    want = oracle.tas_eval(V, PRES, rules, rule_off, prio, cand, flags)
    assert_eval(ctx.tas_eval(gen, rules, rule_off, prio, cand, flags), want, flags, "host")
    assert_eval(eval_device(ctx, gen, rules, rule_off, prio, cand, flags), want, flags, "device")
    if pods and flags & FILTER and with_cand:  # the candidates cut the pass sets
        assert not (want[0] & ~cand).any() and want[0].any()


@pytest.mark.parametrize("strategies,rules_per", [(0, 0), (2, 0), (2, 3)])
def test_tas_violations(ctx, oracle, strategies, rules_per):
    import torch
    gen = set_tas(ctx)
    rules, rule_off, _, _ = make_pods(strategies, rules_per, seed=2)
    want = oracle.tas_violations(V, PRES, rules, rule_off)
    got = ctx.tas_violations(gen, rules, rule_off)
    np.testing.assert_array_equal(got, want)
    viol_t = filled((strategies, W), torch.int64)
    ctx.tas_violations_device(gen, strategies, len(rules), dev(rules), dev(rule_off), viol_t,
                              stream=stream())
    sync()
    np.testing.assert_array_equal(viol_t.cpu().numpy().view(np.uint64), want)
    if strategies and not rules_per:
        assert not want.any()  # a strategy without rules is violated nowhere


@pytest.mark.parametrize("with_labels", [False, True])
@pytest.mark.parametrize("n_nodes,n_strat", [(0, 2), (N, 0), (N, 3)])
def test_tas_label_plan(ctx, oracle, n_nodes, n_strat, with_labels):
    import torch
    rng = np.random.default_rng(3)
    words = w64(n_nodes)
    tail = np.uint64((1 << (n_nodes - 64 * (words - 1))) - 1) if n_nodes else np.uint64(0)
    viol = rng.integers(0, 2**63, (n_strat, words), dtype=np.int64).astype(np.uint64)
    labels = rng.integers(0, 2**63, (n_strat, words), dtype=np.int64).astype(np.uint64)
    if n_nodes:
        viol[:, -1] &= tail
        labels[:, -1] &= tail
    labels = labels if with_labels else None
    want = oracle.label_plan(viol, labels, n_nodes)
    got = ctx.tas_label_plan(n_nodes, viol, labels)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[2] == want[2]
    add_t, rem_t = filled((n_nodes,), torch.int64), filled((n_nodes,), torch.int64)
    total_t = filled((1,), torch.int64)
    ctx.tas_label_plan_device(n_nodes, n_strat, dev(viol), None if labels is None else dev(labels),
                              add_t, rem_t, total_t, stream=stream())
    sync()
    np.testing.assert_array_equal(add_t.cpu().numpy().view(np.uint64), want[0])
    np.testing.assert_array_equal(rem_t.cpu().numpy().view(np.uint64), want[1])
    assert int(total_t.item()) == want[2]
    if n_nodes and n_strat and with_labels:
        assert want[1].any()  # the labels matter: something is removed


def test_tas_prioritize_request_of_no_nodes(ctx, oracle):
    import torch
    gen = set_tas(ctx)
    prio = np.array([(1, 1, 0)], RULE_DTYPE)
    req = np.zeros(0, np.int32)
    want = oracle.prioritize_request(V, PRES, prio[0], req)
    got = ctx.tas_prioritize_request(gen, prio[0], req)
    assert len(want) == 0 and len(got) == 0
    len_t = filled((1,), torch.int32)
    ctx.tas_prioritize_request_device(gen, prio[0], 0, dev(req), filled((1,), torch.int32), len_t,
                                      stream=stream())
    sync()
    assert int(len_t.item()) == 0


@pytest.mark.parametrize("off", [[0, 0, 7], [0, 7, 7]])
def test_tas_prioritize_requests_one_empty(ctx, oracle, off):
    import torch
    gen = set_tas(ctx)
    off = np.array(off, np.int32)
    req = np.array([5, 129, -1, 64, 5, 130, 0], np.int32)
    prio = np.array([(0, 0, 0), (2, 1, 0)], RULE_DTYPE)
    pos, lens = ctx.tas_prioritize_requests(gen, off, prio, req)
    pos_t, len_t = filled((len(req),), torch.int32), filled((2,), torch.int32)
    ctx.tas_prioritize_requests_device(gen, off, prio, dev(req), pos_t, len_t, stream=stream())
    sync()
    np.testing.assert_array_equal(len_t.cpu().numpy(), lens)
    np.testing.assert_array_equal(pos_t.cpu().numpy(), pos)
    for r in range(2):
        want = oracle.prioritize_request(V, PRES, prio[r], req[off[r]:off[r + 1]])
        assert lens[r] == len(want)
        np.testing.assert_array_equal(pos[off[r]:off[r] + lens[r]], want)
        assert (pos[off[r] + lens[r]:off[r + 1]] == -1).all()
    assert 0 in lens and lens.max() > 0


def filter_want(oracle, reqs, rules, rule_off):
    none = np.zeros(len(reqs), RULE_DTYPE)
    none["metric"] = -1
    ok, _, _ = oracle.tas_eval(V, PRES, rules, rule_off, none, flags=FILTER)
    ok = unpack_bits(ok, N)
    return [gather_bits(ok[r], rq, True) for r, rq in enumerate(reqs)]


def filter_device(c, gen, off, rules, rule_off, req, ld):
    out_t = dev(np.full((len(off) - 1, ld), SENTINEL, np.uint64))
    c.tas_filter_requests_device(gen, off, len(rules), dev(rules), dev(rule_off), dev(req), out_t,
                                 ld, stream=stream())
    sync()
    return out_t.cpu().numpy().view(np.uint64)


def test_tas_filter_requests_all_empty(ctx):
    gen = set_tas(ctx)
    rules, rule_off, _, _ = make_pods(2, 2, seed=4)
    off, req = np.zeros(3, np.int32), np.zeros(0, np.int32)
    out = np.full((2, 2), SENTINEL, np.uint64)
    rows = ctx.tas_filter_requests(gen, off, rules, rule_off, req, out=out)
    assert (rows == SENTINEL).all()  # no request has a word
    assert (filter_device(ctx, gen, off, rules, rule_off, req, 2) == SENTINEL).all()


def test_tas_filter_requests_rows_wider_than_the_longest(ctx, oracle):
    gen = set_tas(ctx)
    rng = np.random.default_rng(5)
    reqs = [rng.integers(-1, N + 1, n).astype(np.int32) for n in (70, 0, 1, 129)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in reqs])]).astype(np.int32)
    req = np.concatenate(reqs)
    rules, rule_off, _, _ = make_pods(len(reqs), 2, seed=6)
    want = filter_want(oracle, reqs, rules, rule_off)
    assert 0.05 < np.concatenate(want).mean() < 0.95
    ld = w64(129) + 2
    out = np.full((len(reqs), ld), SENTINEL, np.uint64)
    rows = ctx.tas_filter_requests(gen, off, rules, rule_off, req, out=out)
    check_rows(rows, reqs, want, SENTINEL, "host")  # every word past W64(n_r) keeps the fill
    check_rows(filter_device(ctx, gen, off, rules, rule_off, req, ld), reqs, want, SENTINEL,
               "device")


@pytest.mark.parametrize("wide", [False, True])
def test_tas_snapshot_update_of_no_columns(ctx, oracle, wide):
    gen = set_tas(ctx)
    none = np.zeros(0, np.int32)
    if wide:
        ctx.tas_snapshot_update_wide(gen, gen + 1, none, np.zeros((0, N), np.int64),
                                     np.zeros((0, N), np.uint32), np.zeros((0, W), np.uint64))
        ctx.tas_snapshot_update_wide_device(gen + 1, gen + 2, none, None, None, None,
                                            stream=stream())
    else:
        ctx.tas_snapshot_update(gen, gen + 1, none, np.zeros((0, N), np.int64),
                                np.zeros((0, W), np.uint64))
        ctx.tas_snapshot_update_device(gen + 1, gen + 2, none, None, None, stream=stream())
    sync()
    assert ctx.tas_snapshot_info() == (gen + 2, N, M) and ctx.tas_snapshot_wide_count() == 0
    rules, rule_off, prio, _ = make_pods(3, 2)
    flags = FILTER | PRIORITIZE
    assert_eval(ctx.tas_eval(gen + 2, rules, rule_off, prio), oracle.tas_eval(
        V, PRES, rules, rule_off, prio), flags, "after the update")


def test_scratch_regrowth_between_calls(oracle):
    """The second call's arrays pass the scratch buffer's first size (1 MiB) through order_out
    [2100][130]: the buffer is freed and allocated again after the first call laid its arrays
    out in the old one, and the third call runs in the grown one."""
    with pas_amd.Context(0) as c:
        c.tas_snapshot_set(7, V, PRES)
        assert 2100 * N * 4 > 1 << 20
        for pods in (2, 2100, 2):
            rules, rule_off, prio, cand = make_pods(pods, 2, seed=pods)
            flags = FILTER | PRIORITIZE
            want = oracle.tas_eval(V, PRES, rules, rule_off, prio, cand, flags)
            assert_eval(c.tas_eval(7, rules, rule_off, prio, cand, flags), want, flags,
                        f"{pods} pods")


# ------------------------------------------------------------------------- GAS

N_CARDS = np.array([3, 3, 2, 0, -1], np.int32)
CAP = np.tile(np.array([100, 10_000], np.int64), (GN, 1))
USED = np.array([[[k, 100 * (n + k)] for k in range(GK)] for n in range(GN)], np.int64)
# pod 0: one container of 9 selections (more than the result word packs: a side record on
# every node that takes it); pod 1: two containers, 1 + 2 selections; pod 2: no container
REQ = np.array([[[9, 900], [0, 0]], [[1, 50], [2, 100]], [[0, 0], [0, 0]]], np.int64)
MASK = np.array([[3, 0], [3, 3], [0, 0]], np.uint32)
NCONT = np.array([1, 2, 0], np.int32)
REQ0, MASK0 = np.zeros((3, 0, GQ), np.int64), np.zeros((3, 0), np.uint32)  # max_containers 0
NCONT0 = np.zeros(3, np.int32)
I915 = 0


def set_gas(c):
    _gen[0] += 10
    c.gas_snapshot_set(_gen[0], N_CARDS, CAP, USED)
    return _gen[0]


def assert_gas(c, gen, used):
    assert c.gas_snapshot_info() == (gen, GN, GK, GQ)
    g, after = c.gas_snapshot_get()
    assert g == gen
    np.testing.assert_array_equal(after, used)


def fit_device(c, gen, req, mask, ncont):
    import torch
    res_t = filled((len(ncont), GN), torch.int32)
    c.gas_fit_device(gen, len(ncont), req.shape[1], I915, dev(req), dev(mask), dev(ncont), res_t,
                     stream=stream())
    sync()
    return res_t.cpu().numpy().view(np.uint32)


def test_gas_fit_without_containers(ctx, oracle):
    gen = set_gas(ctx)
    req, mask, ncont = REQ0[:1], MASK0[:1], NCONT0[:1]
    want = oracle.gas_fit(N_CARDS, CAP, USED, req, mask, ncont, I915)
    np.testing.assert_array_equal(ctx.gas_fit(gen, req, mask, ncont, I915), want)
    np.testing.assert_array_equal(fit_device(ctx, gen, req, mask, ncont), want)


def fit_ex_raw(c, gen, side_cap, n_side):
    """pas_gas_fit_ex with exactly side_cap (the binding's gas_fit_ex grows the buffer):
    (words, side [n_side] pre-filled with pod -9, count)."""
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((len(NCONT), GN), np.uint32)
    side = np.zeros(n_side, _lib.GAS_SELECTION_DTYPE)
    side["pod"] = -9
    count = ctypes.c_int64(-1)
    rc = c._l.pas_gas_fit_ex(c._h, gen, len(NCONT), REQ.shape[1], I915, p(REQ), p(MASK),
                             p(NCONT), p(out), p(side) if side_cap else None, side_cap,
                             ctypes.byref(count))
    c._check(rc, "pas_gas_fit_ex")
    return out, side, count.value


def fit_ex_device(c, gen, side_cap, n_side):
    import torch
    res_t = filled((len(NCONT), GN), torch.int32)
    side = np.zeros(n_side, _lib.GAS_SELECTION_DTYPE)
    side["pod"] = -9
    side_t = torch.from_numpy(side.view(np.uint8).reshape(n_side, -1).copy()).cuda()
    count_t = filled((1,), torch.int64)
    c.gas_fit_ex_device(gen, len(NCONT), REQ.shape[1], I915, dev(REQ), dev(MASK), dev(NCONT),
                        res_t, side_t if side_cap else None, side_cap, count_t, stream=stream())
    sync()
    return (res_t.cpu().numpy().view(np.uint32),
            side_t.cpu().numpy().view(_lib.GAS_SELECTION_DTYPE).reshape(-1), int(count_t.item()))


def test_gas_fit_ex_side_capacity(ctx, oracle):
    gen = set_gas(ctx)
    words, sel, nsel = oracle.gas_fit(N_CARDS, CAP, USED, REQ, MASK, NCONT, I915, selections=True)
    ext = np.argwhere(((words >> 31) == 1) & (((words >> 24) & 0xF) == _lib.PAS_GAS_SEL_EXTENDED))
    full = {(int(p), int(n)): bytes(sel[p, n, :nsel[p, n]]) for p, n in ext}
    assert len(full) == 3 and all(len(v) == 9 for v in full.values())
    got_words, got_side = ctx.gas_fit_ex(gen, REQ, MASK, NCONT, I915)
    np.testing.assert_array_equal(got_words, words)
    assert {(int(s["pod"]), int(s["node"])): bytes(s["card"][:s["n_sel"]])
            for s in got_side} == full
    for cap in (0, len(full) - 1):
        for what, run in (("host", fit_ex_raw), ("device", fit_ex_device)):
            w, side, count = run(ctx, gen, cap, len(full))
            np.testing.assert_array_equal(w, words, err_msg=what)
            assert count == len(full), what  # the full count, whatever the capacity
            written = side[side["pod"] != -9]
            assert len(written) == cap and (side["pod"][cap:] == -9).all(), what
            keys = {(int(s["pod"]), int(s["node"])) for s in written}
            assert len(keys) == cap and keys <= set(full), what
            for s in written:
                assert bytes(s["card"][:s["n_sel"]]) == full[int(s["pod"]), int(s["node"])], what


BIND_FORMS = [{}, {"selections": True}, {"counts": True}]


@pytest.mark.parametrize("form", BIND_FORMS, ids=["bind", "bind_ex", "bind_counts"])
def test_gas_bind_of_no_binds(ctx, form):
    gen = set_gas(ctx)
    got = ctx.gas_bind(gen, gen + 1, [], [], REQ, MASK, NCONT, I915, **form)
    assert all(len(a) == 0 for a in got)
    assert_gas(ctx, gen + 1, USED)  # the generation still steps


@pytest.mark.parametrize("form", BIND_FORMS, ids=["bind", "bind_ex", "bind_counts"])
def test_gas_bind_without_containers(ctx, oracle, form):
    gen = set_gas(ctx)
    pods, nodes = [0, 2, 1, 0], [0, 3, 4, 0]
    want = oracle.gas_bind(N_CARDS, CAP, USED, REQ0, MASK0, NCONT0, I915, pods, nodes, **form)
    got = ctx.gas_bind(gen, gen + 1, pods, nodes, REQ0, MASK0, NCONT0, I915, **form)
    assert len(got) == len(want) - 1
    for g, w in zip(got, want[1:]):
        np.testing.assert_array_equal(g, w)
    assert_gas(ctx, gen + 1, want[0])


def test_gas_release_of_no_releases(ctx):
    gen = set_gas(ctx)
    st = ctx.gas_release(gen, gen + 1, [], [], REQ, MASK, NCONT, np.zeros((0, 2), np.int32),
                         np.zeros((0, _lib.PAS_GAS_PACKED), np.int32))
    assert len(st) == 0
    assert_gas(ctx, gen + 1, USED)
    st = ctx.gas_release_counts(gen + 1, gen + 2, [], [], REQ, MASK, NCONT,
                                np.zeros((0, 2, GK), np.int64))
    assert len(st) == 0
    assert_gas(ctx, gen + 2, USED)


def test_gas_release_counts_without_containers(ctx, oracle):
    gen = set_gas(ctx)
    pods, nodes = [1, 0, 2], [0, 4, 3]
    counts = np.zeros((3, 0, GK), np.int64)
    used, want = oracle.gas_release_counts(N_CARDS, USED, REQ0, MASK0, NCONT0, pods, nodes, counts)
    st = ctx.gas_release_counts(gen, gen + 1, pods, nodes, REQ0, MASK0, NCONT0, counts)
    np.testing.assert_array_equal(st, want)
    assert_gas(ctx, gen + 1, used)


@pytest.mark.parametrize("n_pods", [3, 0])
def test_gas_apply_of_no_events(ctx, n_pods):
    import torch
    gen = set_gas(ctx)
    none = np.zeros(0, np.int32)
    req, mask, ncont = REQ[:n_pods], MASK[:n_pods], NCONT[:n_pods]
    st = ctx.gas_apply(gen, gen + 1, none, none, none, req, mask, ncont,
                       np.zeros((0, 2), np.int32), np.zeros((0, 4), np.int32))
    assert len(st) == 0
    assert_gas(ctx, gen + 1, USED)
    ctx.gas_apply_device(gen + 1, gen + 2, 0, dev(none), dev(none), dev(none), n_pods, 2,
                         dev(req), dev(mask), dev(ncont), dev(none), dev(none), 4,
                         filled((0,), torch.int32), stream=stream())
    sync()
    assert_gas(ctx, gen + 2, USED)


ROWS = np.array([[0, 1], [0, 2], [3, 1]], np.int32)
ROW_LEN = np.array([2, 1, 2], np.int32)


def place_device(c, gen, req, mask, ncont, rows, cand_len, selections, counts):
    import torch
    p, cont = req.shape[:2]
    node_t, rank_t, res_t = (filled((p,), torch.int32) for _ in range(3))
    cards_t = filled((p, 64), torch.uint8) if selections else None
    nsel_t = filled((p,), torch.int32) if selections else None
    cnt_t = filled((p, cont, GK), torch.int64) if counts else None
    n_placed, _ = c.gas_place_device(
        gen, gen + 1, p, cont, I915, dev(req), dev(mask), dev(ncont), rows.shape[1],
        rows.shape[1], 0, dev(rows), None if cand_len is None else dev(cand_len), node_t, rank_t,
        res_t, cards_t, nsel_t, cnt_t, stream=stream())
    out = (node_t.cpu().numpy(), rank_t.cpu().numpy(), res_t.cpu().numpy().view(np.uint32),
           n_placed)
    out += (cards_t.cpu().numpy(), nsel_t.cpu().numpy()) if selections else ()
    return out + ((cnt_t.cpu().numpy(),) if counts else ())


def assert_place(got, want, selections, counts, what):
    for g, key in zip(got, ("node", "rank", "res")):
        np.testing.assert_array_equal(g, want[key], err_msg=f"{what}: {key}")
    assert got[3] == want["n_placed"], what
    rest = list(got[4:])
    if selections:
        np.testing.assert_array_equal(rest.pop(0), want["cards"], err_msg=what)
        np.testing.assert_array_equal(rest.pop(0), want["nsel"], err_msg=what)
    if counts:
        np.testing.assert_array_equal(rest.pop(0), want["counts"], err_msg=what)
    assert not rest


@pytest.mark.parametrize("with_len,selections,counts",
                         list(itertools.product([False, True], repeat=3)))
def test_gas_place_optional_arguments(ctx, oracle, with_len, selections, counts):
    cand_len = ROW_LEN if with_len else None
    want = place_oracle(oracle, N_CARDS, CAP, USED, REQ, MASK, NCONT, I915, ROWS, cand_len)
    assert want["n_placed"] == 3 and want["nsel"][0] == 9 and want["rank"][2] == 1
    gen = set_gas(ctx)
    got = ctx.gas_place(gen, gen + 1, REQ, MASK, NCONT, I915, ROWS, cand_len,
                        selections=selections, counts=counts)
    assert_place(got, want, selections, counts, "host")
    assert_gas(ctx, gen + 1, want["used"])
    gen = set_gas(ctx)
    got = place_device(ctx, gen, REQ, MASK, NCONT, ROWS, cand_len, selections, counts)
    assert_place(got, want, selections, counts, "device")
    assert_gas(ctx, gen + 1, want["used"])


def test_gas_place_cand_len_cuts_the_rows(ctx, oracle):
    # with the lengths the answer differs from the one without: they are read, not dropped
    lens = np.array([2, 0, 1], np.int32)
    want = place_oracle(oracle, N_CARDS, CAP, USED, REQ, MASK, NCONT, I915, ROWS, lens)
    assert list(want["node"]) == [0, -1, -1]
    gen = set_gas(ctx)
    got = ctx.gas_place(gen, gen + 1, REQ, MASK, NCONT, I915, ROWS, lens)
    assert_place(got, want, False, False, "host")
    assert_gas(ctx, gen + 1, want["used"])


def test_gas_place_of_no_pods(ctx):
    gen = set_gas(ctx)
    rows = np.zeros((0, 2), np.int32)
    got = ctx.gas_place(gen, gen + 1, REQ[:0], MASK[:0], NCONT[:0], I915, rows, selections=True,
                        counts=True)
    assert [len(a) for a in got[:3]] == [0, 0, 0] and got[3] == 0
    assert_gas(ctx, gen + 1, USED)
    got = place_device(ctx, gen + 1, REQ[:0], MASK[:0], NCONT[:0], rows, None, True, True)
    assert got[3] == 0
    assert_gas(ctx, gen + 2, USED)


def test_gas_nodes_update_of_no_updates(ctx):
    import torch
    gen = set_gas(ctx)
    none = np.zeros(0, np.int32)
    st = ctx.gas_nodes_update(gen, gen + 1, none, none, np.zeros((0, GQ), np.int64),
                              np.zeros((0, GK), np.int32))
    assert len(st) == 0
    assert_gas(ctx, gen + 1, USED)
    ctx.gas_nodes_update_device(gen + 1, gen + 2, 0, None, None, None, None,
                                filled((0,), torch.int32), stream=stream())
    sync()
    assert_gas(ctx, gen + 2, USED)
    g, n_cards, cap = ctx.gas_snapshot_get_nodes()
    np.testing.assert_array_equal(n_cards, N_CARDS)
    np.testing.assert_array_equal(cap, CAP)


def fit_requests_device(c, gen, off, node, req, mask, ncont, ld):
    fit_t = dev(np.full((len(off) - 1, ld), SENTINEL, np.uint64))
    c.gas_fit_requests_device(gen, off, dev(node), req.shape[1], I915, dev(req), dev(mask),
                              dev(ncont), fit_t, ld, stream=stream())
    sync()
    return fit_t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("containers", [0, 2])
def test_gas_fit_requests(ctx, oracle, containers):
    gen = set_gas(ctx)
    req, mask, ncont = (REQ, MASK, NCONT) if containers else (REQ0, MASK0, NCONT0)
    reqs = [np.array([0, 1, 2, 3, 4, 7, -1], np.int32), np.zeros(0, np.int32),
            np.array([4, 2, 2, 0], np.int32)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in reqs])]).astype(np.int32)
    node = np.concatenate(reqs)
    words = oracle.gas_fit(N_CARDS, CAP, USED, req, mask, ncont, I915)
    want = [gather_bits((words[r] >> 31).astype(bool), rq, False) for r, rq in enumerate(reqs)]
    assert np.concatenate(want).any() and not np.concatenate(want).all()
    out = np.full((3, 3), SENTINEL, np.uint64)
    rows = ctx.gas_fit_requests(gen, off, node, req, mask, ncont, I915, out=out)
    check_rows(rows, reqs, want, SENTINEL, "host")
    check_rows(fit_requests_device(ctx, gen, off, node, req, mask, ncont, 3), reqs, want,
               SENTINEL, "device")
    assert_gas(ctx, gen, USED)


def test_gas_fit_requests_all_empty(ctx):
    gen = set_gas(ctx)
    off, node = np.zeros(4, np.int32), np.zeros(0, np.int32)
    out = np.full((3, 2), SENTINEL, np.uint64)
    rows = ctx.gas_fit_requests(gen, off, node, REQ, MASK, NCONT, I915, out=out)
    assert (rows == SENTINEL).all()
    assert (fit_requests_device(ctx, gen, off, node, REQ, MASK, NCONT, 2) == SENTINEL).all()
