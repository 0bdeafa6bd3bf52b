"""Batch placement (pas_gas_place / pas_gas_place_device): the pods of a batch bound in order,
each along its row of candidate nodes, every bind seeing the binds before it
(GASExtender.bindNode called pod after pod, scheduler.go:385-445).

The expected result is the sequential loop of include/pas.h run with oracle.gas_bind, one
(pod, node) pair per call, the usage carried forward.  The *frozen* answer is the same loop
never committing (every pod judged on the usage the call started from): the cases assert, on
the oracle's result, that the two differ, that pods land past their first choice, that some
stay unplaced and that some node takes a whole run of pods: a device path that got any of
those wrong could not hide in them.  The device result is compared bit for bit."""
import functools

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd import workload as wl
from helpers import decode_gas_word, golden
from test_gas_gpu import random_gas
from test_oracle_golden import gas_readme_case

G = golden()
INT32_MAX = 2**31 - 1
# the binding's signatures of the two entry points (argument types)
PLACE_ARGS = _lib.SIGNATURES["pas_gas_place"][1]
PLACE_DEVICE_ARGS = _lib.SIGNATURES["pas_gas_place_device"][1]


def place_oracle(oracle, n_cards, cap, used, req, mask, ncont, i915, cand, cand_len=None,
                 k=None, node_base=0, commit=True):
    """The loop of pas_gas_place with oracle.gas_bind, one pair per call.  commit=False is
    the frozen answer (no bind changes the usage).  Returns a dict: node, rank, res, cards,
    nsel, counts, n_placed, used (after), attempts (oracle calls)."""
    cand = np.asarray(cand, np.int64)
    p_n = req.shape[0]
    n = len(n_cards)
    k = cand.shape[1] if k is None else k
    used = np.array(used, np.int64, copy=True)
    out = {"node": np.full(p_n, -1, np.int32), "rank": np.full(p_n, -1, np.int32),
           "res": np.zeros(p_n, np.uint32), "cards": np.zeros((p_n, 64), np.uint8),
           "nsel": np.zeros(p_n, np.int32),
           "counts": np.zeros((p_n, req.shape[1], used.shape[1]), np.int64), "attempts": 0}
    for p in range(p_n):
        for j in range(min(k, k if cand_len is None else int(cand_len[p]))):
            node = int(cand[p, j]) - node_base
            if node < 0 or node >= n:
                continue
            after, res, st, cards, nsel, cnt = oracle.gas_bind(
                n_cards, cap, used, req, mask, ncont, i915, [p], [node], selections=True,
                counts=True)
            out["attempts"] += 1
            if st[0] == _lib.PAS_GAS_OK:
                if commit:
                    used = after
                out["node"][p], out["rank"][p], out["res"][p] = node + node_base, j, res[0]
                out["cards"][p], out["nsel"][p], out["counts"][p] = cards[0], nsel[0], cnt[0]
                break
    out["n_placed"] = int((out["node"] >= 0).sum())
    out["used"] = used
    return out


def make_rows(rng, p, n, k, hot):
    """Candidate rows [p][k]: k distinct nodes, each drawn from the first `hot` nodes with
    probability 0.7, else from all; in 20 % of rows one later entry repeats the first; in
    10 % one entry is -1, n or INT32_MAX."""
    rows = np.zeros((p, k), np.int32)
    for i in range(p):
        seen = []
        while len(seen) < k:
            v = int(rng.integers(0, hot if rng.random() < 0.7 else n))
            if v not in seen or len(seen) >= n:
                seen.append(v)
        rows[i] = seen
        if k > 1 and rng.random() < 0.2:
            rows[i, rng.integers(1, k)] = rows[i, 0]
        if rng.random() < 0.1:
            rows[i, rng.integers(0, k)] = (-1, n, INT32_MAX)[rng.integers(0, 3)]
    return rows


# name: (seed, random_gas arguments (n, k, q, p, c), extreme, row k, hot)
RECIPES = {
    "A": (0xA1, (300, 4, 2, 400, 2), False, 6, 40),
    "B": (0xB1, (200, 12, 3, 300, 3), False, 8, 30),      # KMAX 16
    "C": (0xC1, (300, 8, 4, 400, 3), True, 16, 40),
    "D": (0xD0, (1, 8, 2, 200, 2), False, 1, 1),          # one node, one run of 200 pods
    # more than 16 cards per node (KMAX 64, card state in scratch): few nodes, and (in case())
    # at most 2 free units per card, so that the nodes fill up while the batch is placed
    "E": (0xE1, (30, 40, 1, 400, 2), False, 8, 6),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, expected, frozen) of a recipe, computed once and shared (never modified)."""
    import oracle
    oracle.load()
    seed, (n, k, q, p, c), extreme, row_k, hot = RECIPES[name]
    rng = np.random.default_rng(seed)
    n_cards, cap, used, req, mask, ncont = random_gas(rng, n, k, q, p, c, extreme)
    if name == "D":
        n_cards = np.array([8], np.int32)
    if name == "E":
        # random usage leaves about half of a node's 40 cards with room for hundreds of pods:
        # no node would ever fill up
        used = np.maximum(used, cap[:, None, :] - rng.integers(0, 3, size=used.shape))
    rows = make_rows(rng, p, n, row_k, hot)
    inputs = dict(n_cards=n_cards, cap=cap, used=used, req=req, mask=mask, ncont=ncont, rows=rows)
    args = (n_cards, cap, used, req, mask, ncont, 0, rows)
    want = place_oracle(oracle, *args)
    frozen = place_oracle(oracle, *args, commit=False)
    assert want["attempts"] <= 6400
    for v in inputs.values():
        v.setflags(write=False)
    return inputs, want, frozen


def assert_conditions(name):
    """The floors a case must meet on the oracle's result so that it cannot hide a failure:
    pods placed past their first choice (not D: one candidate), pods unplaced, pods whose
    node differs from the frozen answer, a node that takes a run of pods."""
    _, want, frozen = case(name)
    p = len(want["node"])
    placed = want["node"][want["node"] >= 0]
    later, unplaced = int((want["rank"] > 0).sum()), int((want["node"] < 0).sum())
    differ = int((want["node"] != frozen["node"]).sum())
    most = int(np.bincount(placed).max()) if len(placed) else 0
    print(name, "rank>0", later, "unplaced", unplaced, "!=frozen", differ, "most", most)
    assert name == "D" or later >= 0.05 * p
    assert unplaced >= 0.05 * p
    assert differ >= 0.01 * p
    assert most >= 8


# ------------------------------------------------------------------ oracle / binding (CPU)

def test_helper_readme_in_turn(oracle):
    # README.md:15-21: three 5 GB pods, each with the row [0], on a 2-GPU 16 GB node -> card0,
    # card1, unplaced; the frozen answer puts all three on card0
    ex = G["G11_gas_readme"]["memory_example"]
    kinds, cards, n_cards, cap, used, req, mask = gas_readme_case(ex)
    req3, mask3 = np.repeat(req, 3, axis=0), np.repeat(mask, 3, axis=0)
    args = (n_cards, cap, used, req3, mask3, np.ones(3, np.int32), 0, np.zeros((3, 1), np.int32))
    want = place_oracle(oracle, *args)
    assert list(want["node"]) == [0, 0, -1] and list(want["rank"]) == [0, 0, -1]
    assert [decode_gas_word(w) for w in want["res"]] == [(True, [0]), (True, [1]), (False, [])]
    assert want["n_placed"] == 2
    frozen = place_oracle(oracle, *args, commit=False)
    assert [decode_gas_word(w) for w in frozen["res"]] == [(True, [0])] * 3
    np.testing.assert_array_equal(frozen["used"], used)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipes_cannot_hide_a_failure(name):
    assert_conditions(name)


def test_symbols_and_signatures():
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "pas_gas_place") and hasattr(lib, "pas_gas_place_device")
    P, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    out = [ctypes.POINTER(i32)] * 2
    want = [P, u64, u64, i32, i32, i32, P, P, P, i32, i32, i32] + [P] * 8 + out
    assert PLACE_ARGS == want
    assert PLACE_DEVICE_ARGS == want + [P]


def test_null_context():
    z = [None, 0, 1, 0, 0, 0, None, None, None, 1, 1, 0] + [None] * 10
    assert pas_amd.LIB.pas_gas_place(*z) == _lib.PAS_EINVAL
    assert pas_amd.LIB.pas_gas_place_device(*z, None) == _lib.PAS_EINVAL


# ------------------------------------------------------------------ device (GPU)

_gen = [12000]


def _upload(ctx, n_cards, cap, used):
    _gen[0] += 2
    ctx.gas_snapshot_set(_gen[0], n_cards, cap, used)
    return _gen[0]


def _check(ctx, gen, got, want):
    node, rank, res, n_placed = got[:4]
    np.testing.assert_array_equal(node, want["node"])
    np.testing.assert_array_equal(rank, want["rank"])
    np.testing.assert_array_equal(res, want["res"])
    assert n_placed == want["n_placed"]
    g, after = ctx.gas_snapshot_get()
    assert g == gen + 1
    np.testing.assert_array_equal(after, want["used"])


def _round_cap(rows, cand_len=None, k=None):
    k = rows.shape[1] if k is None else k
    lens = np.full(len(rows), k) if cand_len is None else np.clip(cand_len, 0, k)
    return int(lens.sum()) + 1


@pytest.mark.gpu
def test_place_readme_in_turn(ctx, oracle):
    ex = G["G11_gas_readme"]["memory_example"]
    kinds, cards, n_cards, cap, used, req, mask = gas_readme_case(ex)
    req3, mask3 = np.repeat(req, 3, axis=0), np.repeat(mask, 3, axis=0)
    rows = np.zeros((3, 1), np.int32)
    gen = _upload(ctx, n_cards, cap, used)
    got = ctx.gas_place(gen, gen + 1, req3, mask3, np.ones(3, np.int32), 0, rows)
    want = place_oracle(oracle, n_cards, cap, used, req3, mask3, np.ones(3, np.int32), 0, rows)
    assert list(got[0]) == [0, 0, -1] and list(got[1]) == [0, 0, -1]
    _check(ctx, gen, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_place_parity(ctx, name):
    assert_conditions(name)
    i, want, _ = case(name)
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])
    got = ctx.gas_place(gen, gen + 1, i["req"], i["mask"], i["ncont"], 0, i["rows"], rounds=True)
    _check(ctx, gen, got, want)
    assert 1 <= got[-1] <= _round_cap(i["rows"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "E"])
def test_place_parity_selections_counts(ctx, name):
    # more than 8 cards per node (KMAX 16, 64), with the selections and the counts
    assert_conditions(name)
    i, want, _ = case(name)
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])
    got = ctx.gas_place(gen, gen + 1, i["req"], i["mask"], i["ncont"], 0, i["rows"],
                        selections=True, counts=True)
    _check(ctx, gen, got, want)
    np.testing.assert_array_equal(got[4], want["cards"])
    np.testing.assert_array_equal(got[5], want["nsel"])
    np.testing.assert_array_equal(got[6], want["counts"])
    assert (got[6][want["node"] < 0] == 0).all() and (got[4][want["node"] < 0] == 0).all()


@pytest.mark.gpu
def test_place_node_base_pitch_and_lengths(ctx, oracle):
    # node_base != 0, ld > k, rows cut short by cand_len (0 too, and lengths outside [0, k],
    # which are read clamped), a row of out-of-range ids only
    i, _, _ = case("A")
    base, k = 1000, 4
    rng = np.random.default_rng(77)
    rows = np.full((len(i["rows"]), 9), INT32_MAX, np.int32)
    rows[:, :6] = np.where((i["rows"] >= 0) & (i["rows"] < 300), i["rows"] + base, i["rows"])
    rows[:, 6:] = rng.integers(base, base + 300, size=(len(rows), 3))  # past k: never read
    rows[5, :] = [-1, base - 1, base + 300, INT32_MAX, 0, 999, base, base, base]
    cand_len = rng.integers(0, k + 1, size=len(rows)).astype(np.int32)
    cand_len[5], cand_len[7], cand_len[9] = k, -3, k + 5
    args = (i["n_cards"], i["cap"], i["used"], i["req"], i["mask"], i["ncont"], 0)
    want = place_oracle(oracle, *args, rows, cand_len, k=k, node_base=base)
    assert want["node"][5] == -1 and want["node"][7] == -1 and 0 < want["n_placed"] < len(rows)
    assert (want["rank"] > 0).any() and want["node"][want["node"] >= 0].min() >= base
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])
    got = ctx.gas_place(gen, gen + 1, i["req"], i["mask"], i["ncont"], 0, rows, cand_len, k=k,
                        node_base=base, rounds=True)
    _check(ctx, gen, got, want)
    assert got[-1] <= _round_cap(rows, cand_len, k)


@pytest.mark.gpu
def test_place_no_pods(ctx):
    i, _, _ = case("A")
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])
    got = ctx.gas_place(gen, gen + 1, np.zeros((0, 2, 2), np.int64), np.zeros((0, 2), np.uint32),
                        np.zeros(0, np.int32), 0, np.zeros((0, 4), np.int32), rounds=True)
    assert [len(a) for a in got[:3]] == [0, 0, 0] and got[3] == 0 and got[4] == 0
    g, after = ctx.gas_snapshot_get()
    assert g == gen + 1
    np.testing.assert_array_equal(after, i["used"])


@pytest.mark.gpu
def test_place_device_form_equals_host_form(ctx):
    import torch
    i, want, _ = case("A")
    p, c = i["req"].shape[:2]
    k = i["rows"].shape[1]
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)
    node_t = torch.empty(p, dtype=torch.int32, device="cuda")
    rank_t = torch.empty(p, dtype=torch.int32, device="cuda")
    res_t = torch.empty(p, dtype=torch.int32, device="cuda")
    cards_t = torch.empty((p, 64), dtype=torch.uint8, device="cuda")
    nsel_t = torch.empty(p, dtype=torch.int32, device="cuda")
    cnt_t = torch.empty((p, c, 4), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()
    n_placed, n_rounds = ctx.gas_place_device(
        gen, gen + 1, p, c, 0, dev(i["req"]), dev(i["mask"].view(np.int32)), dev(i["ncont"]), k,
        k, 0, dev(i["rows"]), None, node_t, rank_t, res_t, cards_t, nsel_t, cnt_t, stream=stream)
    # the call returns when the placement is complete: no synchronize before the read-back
    got = (node_t.cpu().numpy(), rank_t.cpu().numpy(), res_t.cpu().numpy().view(np.uint32),
           n_placed)
    _check(ctx, gen, got, want)
    np.testing.assert_array_equal(cards_t.cpu().numpy(), want["cards"])
    np.testing.assert_array_equal(nsel_t.cpu().numpy(), want["nsel"])
    np.testing.assert_array_equal(cnt_t.cpu().numpy(), want["counts"])
    assert 1 <= n_rounds <= _round_cap(i["rows"])


@pytest.mark.gpu
def test_place_after_topk(ctx, oracle):
    # a small C5: TAS filter + GAS fit + prioritize top 8 per pod, the rows placed as they are
    import torch
    from test_shard import _dev, _rule_tensors, make_case
    n, p, k = 2000, 256, 8
    snap, batch = make_case(0xC5, n, 6, p, 5)
    gs = wl.make_gas_snapshot(n, seed=0xC5)
    gb = wl.make_gas_batch(p, seed=0xC5)
    c = gb.req.shape[1]
    gen = _upload(ctx, gs.n_cards, gs.cap, gs.used)
    ctx.tas_snapshot_set(gen - 1, snap.v_milli, snap.present)
    rules_t, off_t, prio_t, _ = _rule_tensors(batch, None)
    req_t, mask_t, nc_t = _dev(gb.req), _dev(gb.req_mask.view(np.int32)), _dev(gb.n_containers)
    key = torch.empty((p, k), dtype=torch.int64, device="cuda")
    top_node = torch.empty((p, k), dtype=torch.int32, device="cuda")
    top_len = torch.empty(p, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    ctx.tas_gas_topk_device(gen - 1, gen, p, len(batch.rules), rules_t, off_t, prio_t, None, c,
                            wl.I915, req_t, mask_t, nc_t, k, 0, key, top_node, top_len,
                            stream=stream)
    node_t = torch.empty(p, dtype=torch.int32, device="cuda")
    rank_t = torch.empty(p, dtype=torch.int32, device="cuda")
    res_t = torch.empty(p, dtype=torch.int32, device="cuda")
    n_placed, _ = ctx.gas_place_device(gen, gen + 1, p, c, wl.I915, req_t, mask_t, nc_t, k, k, 0,
                                       top_node, top_len, node_t, rank_t, res_t, stream=stream)
    rows, lens = top_node.cpu().numpy(), top_len.cpu().numpy()
    assert lens.max() == k
    want = place_oracle(oracle, gs.n_cards, gs.cap, gs.used, gb.req, gb.req_mask,
                        gb.n_containers, wl.I915, rows, lens)
    assert want["n_placed"] > 0
    got = (node_t.cpu().numpy(), rank_t.cpu().numpy(), res_t.cpu().numpy().view(np.uint32),
           n_placed)
    _check(ctx, gen, got, want)
    # the derived tables were rebuilt: a fit at the new generation sees the placed pods
    fit = ctx.gas_fit(gen + 1, gb.req, gb.req_mask, gb.n_containers, wl.I915)
    np.testing.assert_array_equal(fit, oracle.gas_fit(gs.n_cards, gs.cap, want["used"], gb.req,
                                                      gb.req_mask, gb.n_containers, wl.I915))


@pytest.mark.gpu
def test_place_errors(ctx):
    i, _, _ = case("A")
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])
    args = (i["req"], i["mask"], i["ncont"], 0, i["rows"])
    for kw, code in [(dict(gen_from=gen - 1), _lib.PAS_ESTALE),
                     (dict(gen_from=gen, k=0), _lib.PAS_EINVAL),
                     (dict(gen_from=gen, k=i["rows"].shape[1] + 1), _lib.PAS_EINVAL)]:  # ld < k
        with pytest.raises(pas_amd.PasError) as e:
            ctx.gas_place(kw.pop("gen_from"), gen + 1, *args, **kw)
        assert e.value.code == code
        g, after = ctx.gas_snapshot_get()
        assert g == gen
        np.testing.assert_array_equal(after, i["used"])
