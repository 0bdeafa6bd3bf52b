"""Batch placement to completion (pas_amd/placement.py: place_to_completion).

The reference is the loop of DESIGN.md §3 "Placement to completion" restated on the CPU with
positions instead of cursor records: every pod holds a position in the oracle's filtered,
ordered list; a round gives each queued pod the next k nodes of its list, from its position,
that fit it on the usage of the round's start (oracle.gas_fit); place_oracle (test_gas_place.py,
oracle.gas_bind pod after pod) places the rows; a pod that was not placed and had a full row
continues behind the last node of the row.  The device path must give the same node, round
and result word per pod, the same counts and the same final usage."""
import functools

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd import workload as wl
from test_gas_place import place_oracle
from test_shard import _dev, _rule_tensors, make_case

INT32_MAX = 2**31 - 1
N, P, K = 2000, 256, 8
SEED = 0xC5


def reference(oracle, tas_lists, gs, gb, i915, k, used=None):
    """The placement loop on the CPU.  tas_lists[p]: pod p's ordered list over the nodes that
    pass its TAS filter (no GAS).  Returns a dict: node, round, res [P]; n_placed, rounds,
    used (final); requeued [P] (rounds a pod went back to the queue), short [P] (the pod's last
    row was shorter than k), per_round (pods placed per round)."""
    p_n = len(tas_lists)
    used = np.array(gs.used if used is None else used, np.int64, copy=True)
    pos = np.zeros(p_n, np.int64)
    queued = np.ones(p_n, bool)
    out = dict(node=np.full(p_n, -1, np.int32), round=np.full(p_n, -1, np.int32),
               res=np.zeros(p_n, np.uint32), requeued=np.zeros(p_n, np.int32),
               short=np.zeros(p_n, bool), per_round=[])
    rounds = 0
    while queued.any():
        fit = (oracle.gas_fit(gs.n_cards, gs.cap, used, gb.req, gb.req_mask, gb.n_containers,
                              i915) >> 31).astype(bool)
        rows = np.full((p_n, k), INT32_MAX, np.int32)
        lens = np.zeros(p_n, np.int32)
        for p in np.flatnonzero(queued):
            lst = tas_lists[p][pos[p]:]
            hit = np.flatnonzero(fit[p, lst])[:k]
            rows[p, :len(hit)], lens[p] = lst[hit], len(hit)
            pos[p] += (hit[-1] + 1) if len(hit) == k else len(lst)
        got = place_oracle(oracle, gs.n_cards, gs.cap, used, gb.req, gb.req_mask,
                           gb.n_containers, i915, rows, lens, k=k)
        used = got["used"]
        placed = got["node"] >= 0
        out["node"][placed], out["res"][placed] = got["node"][placed], got["res"][placed]
        out["round"][placed] = rounds
        out["per_round"].append(int(placed.sum()))
        out["short"][queued] = lens[queued] < k
        queued &= ~placed & (lens == k)
        out["requeued"] += queued
        rounds += 1
    out.update(n_placed=int((out["node"] >= 0).sum()), rounds=rounds, used=used)
    return out


@functools.lru_cache(maxsize=None)
def case():
    """The shape of test_place_after_topk (N = 2 000, 256 pods, k = 8) with the capacity
    tightened as recipe E of test_gas_place.py does (usage raised to just under the capacity):
    all but one node in sixteen are left without room for any pod that asks for a GPU, the
    others with room on a card or two, and the pods prioritize two metrics only, so that dozens
    of pods walk the same order and take each other's candidates.  Pods 3 and 4 ask for more
    than any card holds.  Returns (inputs, lists, reference), computed once, never modified."""
    import oracle
    oracle.load()
    snap, batch = make_case(SEED, N, 6, P, 5)
    batch.prio["metric"] %= 2
    gs = wl.make_gas_snapshot(N, seed=SEED)
    gb = wl.make_gas_batch(P, seed=SEED)
    rng = np.random.default_rng(SEED)
    roomy = rng.random(N) < 0.06
    half = rng.integers(0, 2, gs.used.shape) * gs.cap[:, None, :] // 2
    free = np.where(roomy[:, None, None], half, 0)
    gs.used = np.maximum(gs.used, gs.cap[:, None, :] - np.maximum(free, 1))
    gs.used[np.arange(gs.used.shape[1])[None, :] >= gs.n_cards[:, None]] = 0
    gb.req[3:5, 0, :2], gb.req_mask[3:5, 0] = (1, 10**9), 0b111
    _, order, lens = oracle.tas_eval(snap.v_milli, snap.present, batch.rules, batch.rule_off,
                                     batch.prio, None, 3)
    lists = [order[p, :lens[p]].copy() for p in range(P)]
    want = reference(oracle, lists, gs, gb, wl.I915, K)
    for a in (gs.used, gb.req, gb.req_mask, want["used"]):
        a.setflags(write=False)
    return dict(snap=snap, batch=batch, gs=gs, gb=gb), lists, want


def test_case_cannot_hide_a_failure(oracle):
    """Floors on the reference's own result."""
    i, lists, want = case()
    gs, gb = i["gs"], i["gb"]
    fit0 = (oracle.gas_fit(gs.n_cards, gs.cap, gs.used, gb.req, gb.req_mask, gb.n_containers,
                           wl.I915) >> 31).astype(bool)
    nowhere = np.array([not fit0[p, lists[p]].any() for p in range(P)])
    unplaced = want["node"] < 0
    counts = dict(rounds=want["rounds"], requeued=int((want["requeued"] > 0).sum()),
                  placed_later=int((want["round"] > 0).sum()),
                  unplaced_short=int((unplaced & want["short"] & ~nowhere).sum()),
                  nowhere=int(nowhere.sum()), n_placed=want["n_placed"],
                  per_round=want["per_round"])
    print(counts)
    assert counts["rounds"] >= 3
    assert counts["requeued"] >= 0.10 * P
    assert counts["placed_later"] >= 0.05 * P
    assert counts["unplaced_short"] >= 1  # ran out of nodes during the call
    assert counts["nowhere"] >= 1 and unplaced[nowhere].all()  # unplaced from the start
    assert (want["node"][~unplaced] >= 0).all() and want["n_placed"] >= P // 4


# ------------------------------------------------------------------ device (GPU)
_gen = [71000]


def _run(ctx, k, max_rounds=None, gas_gen_offset=0):
    """Both snapshots set afresh, then place_to_completion; returns (result, gas generation
    the call started from)."""
    from pas_amd.placement import place_to_completion
    i, _, _ = case()
    snap, batch, gs, gb = i["snap"], i["batch"], i["gs"], i["gb"]
    _gen[0] += 100
    gen = _gen[0]
    ctx.tas_snapshot_set(gen - 1, snap.v_milli, snap.present)
    ctx.gas_snapshot_set(gen, gs.n_cards, gs.cap, np.array(gs.used))
    rules_t, off_t, prio_t, _ = _rule_tensors(batch, None)
    req_t, mask_t = _dev(np.array(gb.req)), _dev(np.array(gb.req_mask).view(np.int32))
    nc_t = _dev(gb.n_containers)
    args = (gen - 1, gen + gas_gen_offset, P, len(batch.rules), rules_t, off_t, prio_t, None,
            gb.req.shape[1], wl.I915, req_t, mask_t, nc_t, k)
    return (lambda: place_to_completion(ctx, *args, max_rounds=max_rounds)), gen, args


@pytest.fixture(scope="module")
def completed(ctx, oracle):
    """One run of the case, with what the tests read of the context afterwards."""
    i, _, _ = case()
    gb = i["gb"]
    call, gen, _ = _run(ctx, K)
    r = call()
    g, used = ctx.gas_snapshot_get()
    fit = ctx.gas_fit(g, gb.req, gb.req_mask, gb.n_containers, wl.I915)
    return dict(r=r, gen=gen, g=g, used=used, fit=(fit >> 31).astype(bool),
                node=r.node.cpu().numpy(), round=r.round.cpu().numpy(),
                res=r.res.cpu().numpy().view(np.uint32))


@pytest.mark.gpu
def test_parity_with_the_reference_loop(completed):
    _, _, want = case()
    c = completed
    np.testing.assert_array_equal(c["node"], want["node"])
    np.testing.assert_array_equal(c["round"], want["round"])
    np.testing.assert_array_equal(c["res"], want["res"])
    assert c["r"].n_placed == want["n_placed"] and c["r"].rounds == want["rounds"]
    assert c["r"].gas_gen == c["gen"] + want["rounds"] == c["g"]
    np.testing.assert_array_equal(c["used"], want["used"])


@pytest.mark.gpu
def test_completeness(completed):
    """No unplaced pod has a node left that passes its TAS filter and fits it at the final
    generation; every placed pod's node is in its list."""
    _, lists, _ = case()
    c = completed
    for p in range(P):
        if c["node"][p] < 0:
            assert not c["fit"][p, lists[p]].any(), p
        else:
            assert c["node"][p] in lists[p], p
    assert (c["node"] < 0).sum() >= 2


@pytest.mark.gpu
def test_one_round_equals_the_existing_path(ctx):
    """k = the node count, so every row is the pod's whole list: one round, equal to
    pas_gas_place_device on the rows of the entry point without a cursor
    (test_place_after_topk's check)."""
    import torch
    i, lists, _ = case()
    gb = i["gb"]
    k = N
    call, gen, args = _run(ctx, k)
    r = call()
    assert r.rounds == 1 and r.gas_gen == gen + 1
    got = (r.node.cpu().numpy(), r.res.cpu().numpy(), r.n_placed, ctx.gas_snapshot_get()[1])
    assert (r.round.cpu().numpy() == np.where(got[0] >= 0, 0, -1)).all()
    # the existing path on the same snapshots, set afresh
    call, gen, args = _run(ctx, k)
    key = torch.empty((P, k), dtype=torch.int64, device="cuda")
    top_node = torch.empty((P, k), dtype=torch.int32, device="cuda")
    top_len = torch.empty(P, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    ctx.tas_gas_topk_device(*args, 0, key, top_node, top_len, stream=stream)
    node_t = torch.empty(P, dtype=torch.int32, device="cuda")
    rank_t = torch.empty(P, dtype=torch.int32, device="cuda")
    res_t = torch.empty(P, dtype=torch.int32, device="cuda")
    c, i915, req_t, mask_t, nc_t = args[8:13]
    n_placed, _ = ctx.gas_place_device(gen, gen + 1, P, c, i915, req_t, mask_t, nc_t, k, k, 0,
                                       top_node, top_len, node_t, rank_t, res_t, stream=stream)
    np.testing.assert_array_equal(got[0], node_t.cpu().numpy())
    np.testing.assert_array_equal(got[1], np.where(got[0] >= 0, res_t.cpu().numpy(), 0))
    assert got[2] == n_placed and 0 < n_placed < P
    np.testing.assert_array_equal(got[3], ctx.gas_snapshot_get()[1])


@pytest.mark.gpu
def test_failure_modes(ctx):
    i, _, want = case()
    assert want["rounds"] > 1
    call, gen, _ = _run(ctx, K, max_rounds=1)
    with pytest.raises(RuntimeError, match="max_rounds"):
        call()
    assert ctx.gas_snapshot_get()[0] == gen + 1  # the round that ran stays committed
    # a stale GAS generation: PAS_ESTALE with nothing changed
    call, gen, _ = _run(ctx, K, gas_gen_offset=-1)
    with pytest.raises(pas_amd.PasError) as e:
        call()
    assert e.value.code == _lib.PAS_ESTALE
    g, used = ctx.gas_snapshot_get()
    assert g == gen
    np.testing.assert_array_equal(used, i["gs"].used)
