"""Narrow (64-bit) metric columns at the int64 limits, on every path that restates
core.EvaluateRule for them (csrc/pas_internal.h target_scaled and its seven callers) and on
every order that depends on how the limit values sort.  The grid, the two snapshots (27 and
2112 nodes, columns at scales 0..9 and one column no node has) and the oracle's agreement with
the big-integer definition on them are tests/test_narrow_limits_oracle.py; here the kernels
are compared with that oracle (v_scale = the column's scale), bit-exact: every word, every
list entry up to its length, every record.

    eval        ranges_group / fence_bounds            tas_eval, tas_topk[_wide]_device
    sweep       tas_violations_run_kernel [lo, hi]     tas_violations, the fused deschedule,
                                                       tas_deschedule_patches, the policy table
    lazy (a)    compile_rule -> LazyRule, <= 32 rules  tas_gas_topk[_wide]_device
    lazy (b)    the unstaged compare, 33..40 rules     the same
    lazy (c)    half_bounds skip ranges, 1 / 4 / 6     the same
    resume      topk_start_kernel                      the _after forms, place_to_completion
    requests    the FiltRule tile                      tas_filter_requests

The shapes rest on kStageRules = 32, kSkip = 4 and kRuleTile = 64, pinned by
tests/test_launch_constants.py."""
import functools

import numpy as np
import pytest
import torch

from pas_amd import workload as wl
from pas_amd.workload import pack_bits
from helpers import RULE_DTYPE, unpack_bits
from test_labels import _fused_and_separate
from test_launch_shapes import assert_lists, narrow_records
from test_narrow_limits_oracle import (CASES, EQ, GT, I64_MAX, I64_MIN, LT, M, SCALES,
                                       assert_long_shape, grid_targets, limit_strategies,
                                       mixed_batch, single_rules)
from test_patch_list import fused_all_forms
from test_place_complete import reference
from test_request_batch import check_rows, gather_bits
from test_shard import _dev
from test_topk_after import Dev, last_record
from test_topk_wide import expected_records
from test_wide_columns import requests_for

pytestmark = pytest.mark.gpu

I32_MAX, U32_MAX = 2**31 - 1, 2**32 - 1
BASE = 1000  # node_base of the record forms
KINDS = ["small", "long"]
_gen = [83000]


def arrays_of(case):
    return case["v"], case["pres_b"], case["sc"]


def install(ctx, v, pres_b):
    """The snapshot with its columns at SCALES; returns the generation."""
    _gen[0] += 20
    ctx.tas_snapshot_set(_gen[0], v, pack_bits(pres_b), scale=SCALES)
    return _gen[0]


@pytest.fixture(scope="module", autouse=True)
def long_shape_holds():
    """Tie runs longer than 32 and a target's run over position 1024, from the arrays, before
    any GPU call of this module."""
    assert_long_shape(CASES["long"]())


# ------------------------------------------------------------------ the steps
def eval_batches(n):
    r2, o2, p2, c2 = mixed_batch(n)
    return [tuple(np.array(a) for a in single_rules()) + (None,), (r2, o2, p2, pack_bits(c2))]


def check_eval(ctx, oracle, gen, v, pres_b, sc, flags=(1, 2, 3)):
    """tas_eval: the single-rule pod of every (metric, operator, target), prioritize operators
    cycling 0..3 over the rule's metric, then the mixed batch with its candidate mask."""
    pres = pack_bits(pres_b)
    for rules, off, prio, cand in eval_batches(v.shape[1]):
        for f in flags:  # (2 alone: the lists of the candidates, no rule applied)
            want = oracle.tas_eval(v, pres, rules, off, prio, cand, f, v_scale=sc)
            assert_lists(ctx.tas_eval(gen, rules, off, prio, cand, f), want, f)


def request_lists(n, count, cap, seed=0x4E):
    """`count` request node lists of at most `cap` entries with repeated and unknown nodes
    (-1 and ids past the snapshot)."""
    rng = np.random.default_rng(seed)
    base = requests_for(rng, n)
    out = []
    for r in range(count):
        req = np.roll(base[r % 3], 7 * r)[:cap].copy()
        req[r % len(req)] = n + (r % 5)
        out.append(req.astype(np.int32))
    off = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.int32)
    return off, np.concatenate(out), out


def want_request_rows(oracle, v, pres, sc, rules, off, reqs):
    none = np.zeros(len(reqs), RULE_DTYPE)
    none["metric"] = -1
    ok, _, _ = oracle.tas_eval(v, pres, rules, off, none, flags=1, v_scale=sc)
    ok = unpack_bits(ok, v.shape[1])
    return [gather_bits(ok[r], req, True) for r, req in enumerate(reqs)]


def check_sweep(ctx, oracle, gen, v, pres_b, sc, set_table=True):
    """tas_violations over every single rule, the fused deschedule with its label plan and
    tas_deschedule_patches over the 64 limit strategies, then the policy table of the single
    rules: tas_policies_violated, tas_eval_policies, tas_filter_requests_policies."""
    n = v.shape[1]
    pres = pack_bits(pres_b)
    rng = np.random.default_rng(0x5EE)
    rules, off, prio = single_rules()
    want_v = oracle.tas_violations(v, pres, rules, off, v_scale=sc)
    np.testing.assert_array_equal(ctx.tas_violations(gen, rules, off), want_v)
    lr, loff = limit_strategies()
    want_l = oracle.tas_violations(v, pres, lr, loff, v_scale=sc)
    labels = pack_bits(rng.random((64, n)) < 0.5)
    f, sep = _fused_and_separate(ctx, gen, n, 64, lr, loff, labels)
    want = oracle.label_plan(want_l, labels, n)
    for got in (f, sep):
        np.testing.assert_array_equal(got[0], want_l)
        np.testing.assert_array_equal(got[1], want[0])
        np.testing.assert_array_equal(got[2], want[1])
        assert got[3] == want[2]
    fused_all_forms(ctx, oracle, gen, n, lr, loff, want_l, labels, None,
                    pack_bits(rng.random((64, n)) < 0.5), pack_bits(rng.random((64, n)) < 0.5),
                    "limit strategies")
    if set_table:
        ctx.tas_policies_set(np.array(rules), np.array(off), np.array(prio))
    np.testing.assert_array_equal(ctx.tas_policies_violated(gen), want_v)
    ids = np.arange(len(prio), dtype=np.int32)
    assert_lists(ctx.tas_eval_policies(gen, ids),
                 oracle.tas_eval(v, pres, rules, off, prio, None, 3, v_scale=sc))
    roff, rnode, reqs = request_lists(n, len(prio), 150)
    rows = ctx.tas_filter_requests_policies(gen, roff, ids, rnode)
    check_rows(rows, reqs, want_request_rows(oracle, v, pres, sc, rules, off, reqs), None,
               "by policy id")


def nothing_rule(rng):
    """A rule that selects no node of either snapshot, on any column."""
    m = int(rng.integers(0, 10))
    return [(m, LT, I64_MIN), (m, GT, I64_MAX), (10, int(rng.integers(0, 3)), 0),
            (-1, EQ, 0), (M + 2, GT, -5)][int(rng.integers(0, 5))]


def buried(rng, rule, count, at):
    """`count` rules: nothing_rule everywhere but position `at`."""
    out = [nothing_rule(rng) for _ in range(count)]
    out[at] = rule
    return out


def csr(per_pod):
    rules = np.array([r for rl in per_pod for r in rl], RULE_DTYPE)
    off = np.cumsum([0] + [len(rl) for rl in per_pod]).astype(np.int32)
    return rules, off


# ------------------------------------------------------------------ eval, sweep
@pytest.mark.parametrize("kind", KINDS)
def test_eval(ctx, oracle, kind):
    v, pres_b, sc = arrays_of(CASES[kind]())
    check_eval(ctx, oracle, install(ctx, v, pres_b), v, pres_b, sc)


@pytest.mark.parametrize("kind", KINDS)
def test_sweep_and_policy_table(ctx, oracle, kind):
    v, pres_b, sc = arrays_of(CASES[kind]())
    check_sweep(ctx, oracle, install(ctx, v, pres_b), v, pres_b, sc)


# ------------------------------------------------------------------ requests
@pytest.mark.parametrize("kind", KINDS)
def test_filter_requests(ctx, oracle, kind):
    """The FiltRule tile: a request per single rule, then requests of 70 rules (two tiles of
    kRuleTile = 64) of which one, in the second tile, selects nodes."""
    case = CASES[kind]()
    v, pres_b, sc = arrays_of(case)
    n, pres = case["N"], case["pres"]
    gen = install(ctx, v, pres_b)
    rules, off, _ = single_rules()
    roff, rnode, reqs = request_lists(n, len(off) - 1, 150)
    rows = ctx.tas_filter_requests(gen, roff, rules, off, rnode)
    check_rows(rows, reqs, want_request_rows(oracle, v, pres, sc, rules, off, reqs), None,
               "single rule")
    rng = np.random.default_rng(0x70)
    live = [(m, op, t) for m in range(10)
            for op, t in ((GT, I64_MIN), (EQ, I64_MIN), (LT, I64_MIN + 1), (EQ, I64_MAX),
                          (GT, I64_MAX - 1), (LT, I64_MAX), (EQ, 0), (LT, 0))]
    r70, o70 = csr([buried(rng, r, 70, 64 + i % 6) for i, r in enumerate(live)])
    roff, rnode, reqs = request_lists(n, len(live), 150, seed=0x71)
    want = want_request_rows(oracle, v, pres, sc, r70, o70, reqs)
    known = np.concatenate([(q >= 0) & (q < n) for q in reqs])
    assert 0.05 < np.concatenate(want)[known].mean() < 0.95
    check_rows(ctx.tas_filter_requests(gen, roff, r70, o70, rnode), reqs, want, None, "70 rules")


@pytest.mark.parametrize("kind", KINDS)
def test_prioritize_requests(ctx, oracle, kind):
    case = CASES[kind]()
    v, pres_b, sc = arrays_of(case)
    n, pres = case["N"], case["pres"]
    gen = install(ctx, v, pres_b)
    reqs = requests_for(np.random.default_rng(0x9E), n)
    prio = np.array([(m, op, 0) for m in range(M) for op in range(3) for _ in reqs], RULE_DTYPE)
    batch = [reqs[i % 3] for i in range(len(prio))]
    want = [oracle.prioritize_request(v, pres, prio[i], batch[i], v_scale=sc)
            for i in range(len(prio))]
    assert sum(len(w) > 0 for w in want) == 10 * 9
    for i in range(len(prio)):
        np.testing.assert_array_equal(ctx.tas_prioritize_request(gen, prio[i], batch[i]),
                                      want[i], err_msg=f"{prio[i]}")
    off = np.concatenate([[0], np.cumsum([len(x) for x in batch])]).astype(np.int32)
    pos, lens = ctx.tas_prioritize_requests(gen, off, prio, np.concatenate(batch))
    for i, w in enumerate(want):
        assert lens[i] == len(w), i
        np.testing.assert_array_equal(pos[off[i]:off[i] + lens[i]], w, err_msg=f"{prio[i]}")
        assert (pos[off[i] + lens[i]:off[i + 1]] == -1).all(), i


# ------------------------------------------------------------------ records
@functools.lru_cache(maxsize=None)
def canonical(kind):
    """(W, F) of every value (pas.h): W = v // 10^s floored, F = (v mod 10^s) * 10^(9-s)."""
    v = CASES[kind]()["v"]
    W = np.zeros(v.shape, np.int64)
    F = np.zeros(v.shape, np.uint32)
    for m in range(M):
        mult, up = 10**SCALES[m], 10**(9 - SCALES[m])
        for i, x in enumerate(v[m].tolist()):
            W[m, i] = x // mult  # (Python integers: // floors and nothing overflows)
            F[m, i] = (x - (x // mult) * mult) * up
    return W, F


def want_records(kind, prio, order, lens, k, wide):
    """(key, [sub,] node, len) of the first k entries of the oracle's lists, padded as pas.h
    states: key INT64_MAX, sub UINT32_MAX, node INT32_MAX."""
    if wide:
        return expected_records(order, lens, prio, *canonical(kind), k, BASE)
    return narrow_records(CASES[kind]()["v"], prio, order, lens, k, BASE)


def assert_records(got, want, what):
    for g, w, name in zip(got, want, ("key", "sub", "node", "len") if len(want) == 4
                          else ("key", "node", "len")):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def outputs(P, k, wide):
    key = torch.empty((P, k), dtype=torch.int64, device="cuda")
    sub = torch.empty((P, k), dtype=torch.int32, device="cuda")
    node = torch.empty((P, k), dtype=torch.int32, device="cuda")
    ln = torch.empty(P, dtype=torch.int32, device="cuda")
    return (key, sub, node, ln) if wide else (key, node, ln)


def to_host(ctx, outs):
    ctx.synchronize()
    got = [o.cpu().numpy() for o in outs]
    if len(got) == 4:
        got[1] = got[1].view(np.uint32)
    return tuple(got)


@pytest.mark.parametrize("kind", KINDS)
def test_topk_from_the_eval(ctx, oracle, kind):
    """tas_topk_device and tas_topk_wide_device: the first 5 records and every record (k past
    the longest list) of the single-rule pods and of the mixed batch."""
    case = CASES[kind]()
    v, pres_b, sc = arrays_of(case)
    n = case["N"]
    gen = install(ctx, v, pres_b)
    for rules, off, prio, cand in eval_batches(n):
        P = len(prio)
        _, order, lens = oracle.tas_eval(v, case["pres"], rules, off, prio, cand, 3, v_scale=sc)
        assert lens.max() > 5
        tens = (_dev(rules.view(np.uint8)), _dev(off), _dev(prio.view(np.uint8)),
                None if cand is None else _dev(cand.view(np.int64)))
        for k in (5, n + 5):
            for wide in (False, True):
                outs = outputs(P, k, wide)
                fn = ctx.tas_topk_wide_device if wide else ctx.tas_topk_device
                fn(gen, P, len(rules), *tens, k, BASE, *outs)
                assert_records(to_host(ctx, outs), want_records(kind, prio, order, lens, k, wide),
                               f"k {k} wide {wide}")


# ------------------------------------------------------------------ lazy top-k
def roomy_gas(n, pods):
    """A GAS snapshot and a pod batch on which every pod fits every node."""
    per_gpu = np.array([300, 1000, 16_000_000_000], np.int64)
    gs = wl.GasSnapshotData(np.full(n, 8, np.int32), np.tile(per_gpu, (n, 1)),
                            np.zeros((n, 8, 3), np.int64))
    req = np.zeros((pods, 1, 3), np.int64)
    req[:, 0] = (1, 10, 10**8)
    return gs, wl.GasBatch(req, np.full((pods, 1), 0b111, np.uint32), np.ones(pods, np.int32))


def batch_staged():
    """(a) one rule per pod (<= kStageRules: compiled into LDS), every grid rule; the pods
    prioritize the rule's metric or the next one, in blocks of four operators 0..3."""
    rules, off, prio = (np.array(a) for a in single_rules())
    other = (np.arange(len(prio)) // 4) % 2 == 1
    prio["metric"][other] = (prio["metric"][other] + 1) % 10
    return rules, off, prio


def batch_unstaged():
    """(b) 33..40 rules per pod, every pod (the staging decision is a ballot over the wave):
    every grid rule once, buried among rules that select nothing."""
    rng = np.random.default_rng(0xB)
    rules, _, prio = batch_staged()
    per_pod = []
    for p, r in enumerate(rules.tolist()):
        count = 33 + p % 8
        per_pod.append(buried(rng, r, count, int(rng.integers(0, count))))
    return csr(per_pod) + (prio,)


def batch_own_metric():
    """(c) 1, 4 and 6 rules (kSkip = 4), all on the pod's prioritize metric, for every column,
    both sorted orders and the index order.  Variant 0: Equals rules on distinct targets
    (narrow ranges); 1: any operator and target of the grid; 2: among them LessThan INT64_MIN
    (an empty range) and rules at the limits that take the whole column or all but its ends."""
    rng = np.random.default_rng(0xC)
    per_pod, prio = [], []
    for m in range(10):
        ts = grid_targets(m)
        for op in (LT, GT, EQ):
            for count in (1, 4, 6):
                for variant in range(3):
                    pick = [ts[i] for i in rng.permutation(len(ts))[:count]]
                    if variant == 0:
                        rl = [(m, EQ, t) for t in pick]
                    else:
                        rl = [(m, int(rng.integers(0, 3)), t) for t in pick]
                    if variant == 2:
                        rl[0] = [(m, LT, I64_MIN), (m, GT, I64_MIN), (m, LT, I64_MAX),
                                 (m, EQ, I64_MIN), (m, GT, I64_MAX)][int(rng.integers(0, 5))]
                    per_pod.append(rl)
                    prio.append((m, op, 0))
    return csr(per_pod) + (np.array(prio, RULE_DTYPE),)


BATCHES = {"staged": batch_staged, "unstaged": batch_unstaged, "own_metric": batch_own_metric}


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("kind", KINDS)
def test_lazy_topk(ctx, oracle, kind, batch):
    """tas_gas_topk_device and the wide form where every pod fits every node: the first k of
    the TAS lists; then the same lists by policy id (tas_topk_policies_device,
    tas_gas_topk_policies_device) with the batch as the policy table."""
    case = CASES[kind]()
    v, sc, n = case["v"], case["sc"], case["N"]
    rules, off, prio = BATCHES[batch]()
    P = len(prio)
    counts = np.diff(off)
    if batch == "staged":
        assert counts.max() <= 32
    elif batch == "unstaged":
        assert counts.min() >= 33 and counts.max() == 40
    else:
        assert set(counts.tolist()) == {1, 4, 6}
    _, order, lens = oracle.tas_eval(v, case["pres"], rules, off, prio, None, 3, v_scale=sc)
    # lists that are whole columns, cut short and empty; all three orders among the non-empty
    assert (lens == 0).any() and (lens > n // 2).any() and ((lens > 0) & (lens < n // 2)).any()
    assert {LT, GT, EQ} <= set(prio["op"][lens > 5].tolist())
    gs, gb = roomy_gas(n, P)
    dev = Dev(ctx, dict(v=v, pres=case["pres"], rules=rules, off=off, prio=prio, cand=None,
                        gs=gs, gb=gb, i915=0), scale=SCALES, wide={})
    for k in (5, n + 5):
        for wide in (False, True):
            assert_records(dev.topk(k, BASE, wide=wide),
                           want_records(kind, prio, order, lens, k, wide),
                           f"k {k} wide {wide}")
    ctx.tas_policies_set(rules, off, prio)
    ids = _dev(np.arange(P, dtype=np.int32))
    for k in (5, n + 5):
        want = want_records(kind, prio, order, lens, k, False)
        outs = outputs(P, k, False)
        ctx.tas_topk_policies_device(dev.tas_gen, P, ids, None, k, BASE, *outs)
        assert_records(to_host(ctx, outs), want, f"topk by policy id, k {k}")
        outs = outputs(P, k, False)
        ctx.tas_gas_topk_policies_device(dev.tas_gen, dev.gas_gen, P, ids, None, *dev.gas, k,
                                         BASE, *outs)
        assert_records(to_host(ctx, outs), want, f"gas topk by policy id, k {k}")


# ------------------------------------------------------------------ resume
def resume_case():
    """Small snapshot: every column (the empty one too) under LessThan, GreaterThan and Equals;
    each pod has one rule, on the next column (Equals 0: it takes a node or two away)."""
    case = CASES["small"]()
    prio = np.array([(m, op, 0) for m in range(M) for op in (LT, GT, EQ)], RULE_DTYPE)
    rules = np.array([((m + 1) % 10, EQ, 0) for m, _, _ in prio.tolist()], RULE_DTYPE)
    off = np.arange(len(prio) + 1, dtype=np.int32)
    gs, gb = roomy_gas(case["N"], len(prio))
    return dict(v=case["v"], pres=case["pres"], rules=rules, off=off, prio=prio, cand=None,
                gs=gs, gb=gb, i915=0)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("k", [4, 1])
def test_resumed_pages_are_the_whole_list(ctx, oracle, k, wide):
    """Pages of k from the begin cursor until a page is empty, each page's last record (padding
    included) the next cursor: their concatenation is the oracle's list, each node once.  With
    k = 1 every record is a cursor: the GreaterThan records of value INT64_MIN and the LessThan
    records of value INT64_MAX (key INT64_MAX, the padding's key), and every position of a tie
    run."""
    c = resume_case()
    case = CASES["small"]()
    n, P = case["N"], len(c["prio"])
    _, order, lens = oracle.tas_eval(c["v"], c["pres"], c["rules"], c["off"], c["prio"], None, 3,
                                     v_scale=case["sc"])
    full = want_records("small", c["prio"], order, lens, n, wide)
    dev = Dev(ctx, c, scale=SCALES, wide={})
    cur = (np.full(P, I64_MIN),) + ((np.zeros(P, np.uint32),) if wide else ()) + \
        (np.full(P, -1),)
    got = [[] for _ in range(P)]
    real_at_max_key = set()
    for _ in range(-(-n // k) + 1):
        page = dev.topk(k, BASE, after=cur, wide=wide)
        ln = page[-1]
        for p in range(P):
            got[p] += list(zip(*(a[p, :ln[p]].tolist() for a in page[:-1])))
            assert (page[0][p, ln[p]:] == I64_MAX).all() and (page[-2][p, ln[p]:] == I32_MAX).all()
            if wide:
                assert (page[1][p, ln[p]:] == U32_MAX).all()
        cur = last_record(page, k)
        real = (cur[0] == I64_MAX) & (cur[-1] != I32_MAX)
        real_at_max_key |= {int(c["prio"]["op"][p]) for p in np.nonzero(real)[0]}
        if not ln.any():
            break
    assert not ln.any()
    for p in range(P):
        want = list(zip(*(a[p, :full[-1][p]].tolist() for a in full[:-1])))
        assert got[p] == want, (p, c["prio"][p])
        assert len({r[-1] for r in got[p]}) == len(got[p])
    if k == 1:  # (the wide key of a scale-0 value is the value's own)
        assert real_at_max_key == {LT, GT}
    # the scale-0 column ties on several nodes, the index order on all of them
    v0 = case["v"][0][case["pres_b"][0]]
    assert len(np.unique(v0)) < len(v0)


def test_place_to_completion(ctx, oracle):
    """40 pods on the small snapshot with room for one pod per node: the placements equal the
    pod-after-pod loop (test_place_complete.reference) on the oracle's lists."""
    from pas_amd.placement import place_to_completion
    case = CASES["small"]()
    n, P, k = case["N"], 40, 4
    rng = np.random.default_rng(0x40)
    rules, off, _ = single_rules()
    pick = rng.permutation(len(rules))[:P]
    rules, off = np.array(rules[pick]), np.arange(P + 1, dtype=np.int32)
    prio = np.array([(p % M, p % 3, 0) for p in range(P)], RULE_DTYPE)
    gs, gb = roomy_gas(n, P)
    gs.n_cards[:] = 1
    gb.req[:, 0, 1] = 1000  # a whole card's millicores: one pod per node
    _, order, lens = oracle.tas_eval(case["v"], case["pres"], rules, off, prio, None, 3,
                                     v_scale=case["sc"])
    lists = [order[p, :lens[p]].copy() for p in range(P)]
    want = reference(oracle, lists, gs, gb, 0, k)
    assert want["rounds"] >= 2 and 0 < want["n_placed"] <= n < P
    assert (want["requeued"] > 0).any()
    tas_gen = install(ctx, case["v"], case["pres_b"])
    ctx.gas_snapshot_set(tas_gen + 1, gs.n_cards, gs.cap, gs.used)
    r = place_to_completion(ctx, tas_gen, tas_gen + 1, P, len(rules), _dev(rules.view(np.uint8)),
                            _dev(off), _dev(prio.view(np.uint8)), None, 1, 0, _dev(gb.req),
                            _dev(gb.req_mask.view(np.int32)), _dev(gb.n_containers), k)
    np.testing.assert_array_equal(r.node.cpu().numpy(), want["node"])
    np.testing.assert_array_equal(r.round.cpu().numpy(), want["round"])
    np.testing.assert_array_equal(r.res.cpu().numpy().view(np.uint32), want["res"])
    assert r.n_placed == want["n_placed"] and r.rounds == want["rounds"]
    np.testing.assert_array_equal(ctx.gas_snapshot_get()[1], want["used"])


# ------------------------------------------------------------------ movers (long snapshot)
def check_resident(ctx, v, pres_b):
    """The columns kept their scales and the values where a node has them."""
    _, vals, present, scale, wide, _ = ctx.tas_snapshot_get()
    assert scale.tolist() == SCALES and not wide.any()
    np.testing.assert_array_equal(unpack_bits(present, v.shape[1]), pres_b)
    np.testing.assert_array_equal(vals[pres_b], v[pres_b])


def test_after_column_update(ctx, oracle):
    """tas_snapshot_update of columns 0, 3 and 9 with their values on other nodes; the policy
    table set before the update answers for the new values."""
    v, pres_b, sc = arrays_of(CASES["long"]())
    gen = install(ctx, v, pres_b)
    ctx.tas_policies_set(*(np.array(a) for a in single_rules()))
    rng = np.random.default_rng(0x0309)
    v, pres_b, cols = v.copy(), pres_b.copy(), [0, 3, 9]
    for m in cols:
        perm = rng.permutation(v.shape[1])
        v[m], pres_b[m] = v[m][perm], pres_b[m][perm]
    ctx.tas_snapshot_update(gen, gen + 1, cols, v[cols], pack_bits(pres_b[cols]))
    check_resident(ctx, v, pres_b)
    check_eval(ctx, oracle, gen + 1, v, pres_b, sc)
    check_sweep(ctx, oracle, gen + 1, v, pres_b, sc, set_table=False)


def test_after_reshape(ctx, oracle):
    """tas_snapshot_reshape to 2200 nodes: the row pitch goes from 3072 to 4096."""
    v, pres_b, _ = arrays_of(CASES["long"]())
    gen = install(ctx, v, pres_b)
    n = 2200
    ctx.tas_snapshot_reshape(gen, gen + 1, n, M)
    grown = n - v.shape[1]
    v = np.concatenate([v, np.zeros((M, grown), np.int64)], 1)
    pres_b = np.concatenate([pres_b, np.zeros((M, grown), bool)], 1)
    sc = np.repeat(np.array(SCALES, np.int8)[:, None], n, 1)
    check_resident(ctx, v, pres_b)
    check_eval(ctx, oracle, gen + 1, v, pres_b, sc)
    check_sweep(ctx, oracle, gen + 1, v, pres_b, sc)


def test_after_compact(ctx, oracle):
    """tas_snapshot_compact dropping every third node."""
    v, pres_b, _ = arrays_of(CASES["long"]())
    gen = install(ctx, v, pres_b)
    keep = np.nonzero(np.arange(v.shape[1]) % 3 != 2)[0]
    ctx.tas_snapshot_compact(gen, gen + 1, keep)
    v, pres_b = np.ascontiguousarray(v[:, keep]), np.ascontiguousarray(pres_b[:, keep])
    sc = np.repeat(np.array(SCALES, np.int8)[:, None], len(keep), 1)
    check_resident(ctx, v, pres_b)
    check_eval(ctx, oracle, gen + 1, v, pres_b, sc)
    check_sweep(ctx, oracle, gen + 1, v, pres_b, sc)
