"""pas_gas_snapshot_compact: node rows dropped and renumbered on the device.

N = 130 rows at both register tiers of the row writers (max_cards 8 and 16), Q = 3, random
usage, some rows deleted (n_cards -1, a few of them still with usage), compacted to 100 rows
with -1 gaps.  The read-backs equal the host gather, the fit equals the oracle on the gathered
rows, and a bind after the compaction lands in the row the map gave its node."""
import itertools

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd import workload as wl

N0, N1, P = 130, 100, 12
_gen = itertools.count(0x6C70000, 16)


def rows_for(k, seed):
    gs = wl.make_gas_snapshot(N0, seed=seed, k=k, var_cards=True)
    n_cards, cap, used = gs.n_cards.copy(), gs.cap.copy(), gs.used.copy()
    rng = np.random.default_rng(seed)
    gone = rng.permutation(N0)[:12]
    n_cards[gone] = -1          # deleted nodes: every card parked,
    used[gone[6:]] = 0          # half of them without usage
    return n_cards, cap, used


def node_map(seed):
    """88 of the 130 rows in order, and 12 spare rows among them."""
    rng = np.random.default_rng(seed)
    src = np.sort(rng.permutation(N0)[:N1 - 12])
    for at in np.sort(rng.permutation(N1)[:12]):
        src = np.insert(src, min(at, len(src)), -1)
    assert len(src) == N1 and (np.diff(src[src >= 0]) > 0).all()
    return src.astype(np.int32)


def gathered(src, n_cards, cap, used):
    keep = src >= 0
    at = np.where(keep, src, 0)
    return (np.where(keep, n_cards[at], -1).astype(np.int32),
            np.where(keep[:, None], cap[at], 0), np.where(keep[:, None, None], used[at], 0))


def check_state(ctx, gen, n_cards, cap, used):
    assert ctx.gas_snapshot_info() == (gen,) + used.shape
    g, got_used = ctx.gas_snapshot_get()
    g2, got_nc, got_cap = ctx.gas_snapshot_get_nodes()
    assert g == gen and g2 == gen
    np.testing.assert_array_equal(got_used, used)
    np.testing.assert_array_equal(got_nc, n_cards)
    np.testing.assert_array_equal(got_cap, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 16])
def test_compact_equals_the_host_gather(ctx, oracle, k):
    gen = next(_gen)
    n_cards, cap, used = rows_for(k, 40 + k)
    gb = wl.make_gas_batch(P, seed=k)
    ctx.gas_snapshot_set(gen, n_cards, cap, used)
    ctx.gas_fit(gen, gb.req, gb.req_mask, gb.n_containers, wl.I915)  # derived data exists
    src = node_map(k)
    ctx.gas_snapshot_compact(gen, gen + 1, src)
    assert ctx.gas_shape == (N1, k, 3)
    w_nc, w_cap, w_used = gathered(src, n_cards, cap, used)
    check_state(ctx, gen + 1, w_nc, w_cap, w_used)
    got = ctx.gas_fit(gen + 1, gb.req, gb.req_mask, gb.n_containers, wl.I915)
    want = oracle.gas_fit(w_nc, w_cap, w_used, gb.req, gb.req_mask, gb.n_containers, wl.I915)
    np.testing.assert_array_equal(got, want)
    assert (got >> 31).any() and not (got[:, src < 0] >> 31).any()
    # binds after it: on moved rows, on a spare row and on a deleted node's row
    live = np.flatnonzero((src >= 0) & (w_nc > 0))
    moved = live[src[live] != live]
    nodes = np.concatenate([moved[:6], np.flatnonzero(src < 0)[:1],
                            np.flatnonzero((src >= 0) & (w_nc < 0))[:1]]).astype(np.int32)
    pods = np.arange(len(nodes), dtype=np.int32)
    res, st = ctx.gas_bind(gen + 1, gen + 2, pods, nodes, gb.req, gb.req_mask, gb.n_containers,
                           wl.I915)
    b_used, b_res, b_st = oracle.gas_bind(w_nc, w_cap, w_used, gb.req, gb.req_mask,
                                          gb.n_containers, wl.I915, pods, nodes)
    np.testing.assert_array_equal(st, b_st)
    np.testing.assert_array_equal(res, b_res)
    assert (b_used != w_used).any(axis=(1, 2)).sum() > 0
    check_state(ctx, gen + 2, w_nc, w_cap, b_used)


@pytest.mark.gpu
def test_shrink_to_nothing_grow_and_identity(ctx):
    gen = next(_gen)
    n_cards, cap, used = rows_for(8, 3)
    ctx.gas_snapshot_set(gen, n_cards, cap, used)
    # the identity map moves the generation only
    ctx.gas_snapshot_compact(gen, gen + 1, np.arange(N0))
    check_state(ctx, gen + 1, n_cards, cap, used)
    # larger than the resident count: spare rows behind the kept ones
    src = np.concatenate([np.arange(0, N0, 2), np.full(200, -1)]).astype(np.int32)
    ctx.gas_snapshot_compact(gen + 1, gen + 2, src)
    check_state(ctx, gen + 2, *gathered(src, n_cards, cap, used))
    # and no row at all
    ctx.gas_snapshot_compact(gen + 2, gen + 3, [])
    assert ctx.gas_snapshot_info() == (gen + 3, 0, 8, 3)


@pytest.mark.gpu
def test_refusals_leave_the_snapshot(ctx):
    gen = next(_gen)
    n_cards, cap, used = rows_for(8, 5)
    ctx.gas_snapshot_set(gen, n_cards, cap, used)
    bad = [((gen + 1, gen + 2, [0, 1, 2]), _lib.PAS_ESTALE),
           ((gen, gen + 1, [0, 2, 1]), _lib.PAS_EINVAL),         # not increasing
           ((gen, gen + 1, [0, 1, -1, 1]), _lib.PAS_EINVAL),     # a row twice
           ((gen, gen + 1, [128, 129, 130]), _lib.PAS_EINVAL),   # >= n_nodes
           ((gen, gen + 1, [0, -2, 1]), _lib.PAS_EINVAL)]        # < -1
    for args, code in bad:
        with pytest.raises(pas_amd.PasError) as e:
            ctx.gas_snapshot_compact(*args)
        assert e.value.code == code, args
        ctx.gas_shape = (N0, 8, 3)  # (the handle's shape follows successful calls only)
        check_state(ctx, gen, n_cards, cap, used)


@pytest.mark.gpu
def test_no_snapshot_is_enosnap():
    with pas_amd.Context(0) as fresh:
        with pytest.raises(pas_amd.PasError) as e:
            fresh.gas_snapshot_compact(1, 2, [0])
        assert e.value.code == _lib.PAS_ENOSNAP
