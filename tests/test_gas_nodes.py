"""Node events on the resident GAS snapshot (pas_gas_nodes_update[_device]) and its growth in
place (pas_gas_snapshot_resize).

The reference fetches the node on every fit (scheduler.go:282-300) and keeps the usage by node
and card name (node_resource_cache.go:259-272): a node event changes what the next fit sees and
moves no usage.  Here it rewrites the node's row.  The checker is a numpy replay of the updates
in call order (gather of the old row through upd_src) and the oracle's fit / bind on the
replayed arrays.

Shapes: N = 130 nodes (three waves, no multiple of 64); (K, Q) = (8, 3), (16, 4), (40, 2): the
row in registers, in registers, in scratch; 24 pods of 1-3 containers, some with numI915 > 1.
Batches of U = 0, 1, 70 and 300 updates; the larger ones repeat nodes, and 300 is more than
one workgroup of the update kernel (256 sorted positions)."""
import functools

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib

N, P, C = 130, 24, 3
SHAPES = [(8, 3), (16, 4), (40, 2)]
OK, ERR_INPUT = _lib.PAS_GAS_OK, _lib.PAS_GAS_ERR_INPUT
ADD, REMOVE = _lib.PAS_GAS_EV_ADD, _lib.PAS_GAS_EV_REMOVE
I32_MIN = -2**31

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ inputs and the replay

def snapshot_for(k, q, seed):
    """n_cards in [-1, k] with every value present, capacities that fit a few pods per card,
    usage in every slot: the parked slots (at and past n_cards) are not zero."""
    rng = np.random.default_rng(seed)
    n_cards = rng.integers(-1, k + 1, size=N).astype(np.int32)
    n_cards[:4] = [k, 0, -1, max(k - 1, 1)]
    cap = rng.integers(500, 5000, size=(N, q)).astype(np.int64)
    cap[:, 0] = rng.integers(1, 5, size=N)  # i915 per card
    used = (rng.random((N, k, q)) * cap[:, None, :] * 1.1).astype(np.int64)
    return n_cards, cap, used


@functools.lru_cache(maxsize=None)
def pods_for(q):
    rng = np.random.default_rng(77 + q)
    ncont = rng.integers(1, C + 1, size=P).astype(np.int32)
    req = rng.integers(10, 1500, size=(P, C, q)).astype(np.int64)
    ni = rng.choice([0, 1, 2, 3], size=(P, C), p=[0.1, 0.6, 0.2, 0.1])
    req[:, :, 0] = ni
    mask = np.full((P, C), (1 << q) - 2, np.uint32) | (ni > 0).astype(np.uint32)
    live = np.arange(C)[None, :] < ncont[:, None]
    mask[~live] = 0
    req[~live] = 0
    for a in (req, mask, ncont):
        a.setflags(write=False)
    return req, mask, ncont


def random_updates(k, q, n_upd, seed, pool=None):
    """n_upd updates over `pool` nodes (default: about n_upd / 3 of them, so nodes repeat):
    any card count, new capacities, upd_src a random permutation with holes (-1)."""
    rng = np.random.default_rng(seed)
    if pool is None:
        pool = rng.choice(N, size=min(N, max(1, n_upd // 3)), replace=False)
    nodes = rng.choice(pool, size=n_upd).astype(np.int32)
    ncs = rng.integers(-1, k + 1, size=n_upd).astype(np.int32)
    caps = rng.integers(0, 5000, size=(n_upd, q)).astype(np.int64)
    caps[:, 0] = rng.integers(0, 5, size=n_upd)
    src = np.stack([rng.permutation(k) for _ in range(n_upd)]).astype(np.int32) \
        if n_upd else np.zeros((0, k), np.int32)
    src[rng.random(src.shape) < 0.2] = -1
    return nodes, ncs, caps, src


def replay(n_cards, cap, used, nodes, ncs, caps, src):
    """The updates in call order on copies: (n_cards, cap, used, statuses).  An update whose
    node or count is out of range changes nothing; a src outside [0, K) is zero usage."""
    n_cards, cap, used = n_cards.copy(), cap.copy(), used.copy()
    n, k, _ = used.shape
    st = np.zeros(len(nodes), np.int32)
    for u, node in enumerate(nodes):
        if not (0 <= node < n and -1 <= ncs[u] <= k):
            st[u] = ERR_INPUT
            continue
        old = used[node].copy()  # the whole old row is read before any slot is written
        for slot in range(k):
            s = int(src[u, slot])
            used[node, slot] = old[s] if 0 <= s < k else 0
        n_cards[node], cap[node] = ncs[u], caps[u]
    return n_cards, cap, used, st


_gen = [91000]


def _upload(ctx, n_cards, cap, used):
    _gen[0] += 20
    ctx.gas_snapshot_set(_gen[0], n_cards, cap, used)
    return _gen[0]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _update_device(ctx, gen, nodes, ncs, caps, src):
    import torch
    u = len(nodes)
    st_t = torch.full((max(u, 1),), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    ctx.gas_nodes_update_device(gen, gen + 1, u, _dev(nodes), _dev(ncs), _dev(caps), _dev(src),
                                st_t, stream=stream)
    stream.synchronize()
    return st_t.cpu().numpy()[:u]


def _state(ctx):
    g, used = ctx.gas_snapshot_get()
    g2, n_cards, cap = ctx.gas_snapshot_get_nodes()
    assert g == g2
    return g, n_cards, cap, used


def _check_state(ctx, gen, n_cards, cap, used):
    g, got_nc, got_cap, got_used = _state(ctx)
    assert g == gen
    np.testing.assert_array_equal(got_nc, n_cards)
    np.testing.assert_array_equal(got_cap, cap)
    np.testing.assert_array_equal(got_used, used)


def _check_fit(ctx, oracle, gen, n_cards, cap, used):
    req, mask, ncont = pods_for(used.shape[2])
    got = ctx.gas_fit(gen, req, mask, ncont, 0)
    want = oracle.gas_fit(n_cards, cap, used, req, mask, ncont, 0)
    np.testing.assert_array_equal(got, want)
    return got


# ------------------------------------------------------------------ 1. parity

@pytest.mark.parametrize("k,q", SHAPES)
@pytest.mark.parametrize("n_upd", [0, 1, 70, 300])
def test_update_matches_the_replay_and_the_oracle(ctx, oracle, k, q, n_upd):
    n_cards, cap, used = snapshot_for(k, q, 11 * k)
    upd = random_updates(k, q, n_upd, 500 + k + n_upd)
    w_nc, w_cap, w_used, w_st = replay(n_cards, cap, used, *upd)
    assert not w_st.any()
    # host form
    gen = _upload(ctx, n_cards, cap, used)
    st = ctx.gas_nodes_update(gen, gen + 1, *upd)
    np.testing.assert_array_equal(st, w_st)
    _check_state(ctx, gen + 1, w_nc, w_cap, w_used)
    host_words = _check_fit(ctx, oracle, gen + 1, w_nc, w_cap, w_used)
    assert ctx.gas_snapshot_info() == (gen + 1, N, k, q)
    # _device form: the same statuses, arrays and words
    gen = _upload(ctx, n_cards, cap, used)
    st = _update_device(ctx, gen, *upd)
    np.testing.assert_array_equal(st, w_st)
    _check_state(ctx, gen + 1, w_nc, w_cap, w_used)
    np.testing.assert_array_equal(_check_fit(ctx, oracle, gen + 1, w_nc, w_cap, w_used),
                                  host_words)


# ------------------------------------------------------------------ 2. in-place hazards

@pytest.mark.parametrize("k,q", SHAPES)
def test_permutations_read_the_old_row(ctx, k, q):
    n_cards, cap, used = snapshot_for(k, q, 13 * k)
    swap = np.arange(k)
    swap[[0, k - 1]] = [k - 1, 0]
    rows = {5: (np.arange(k) + 1) % k,   # rotation: every slot's source is overwritten later
            64: swap,                     # a swap
            65: np.arange(k),             # identity
            129: np.full(k, -1)}          # all zero
    nodes = np.array(list(rows), np.int32)
    src = np.stack(list(rows.values())).astype(np.int32)
    ncs, caps = n_cards[nodes], cap[nodes]
    gen = _upload(ctx, n_cards, cap, used)
    st = ctx.gas_nodes_update(gen, gen + 1, nodes, ncs, caps, src)
    assert not st.any()
    want = used.copy()
    for node, s in rows.items():
        want[node] = np.where((s >= 0)[:, None], used[node][np.maximum(s, 0)], 0)
    _check_state(ctx, gen + 1, n_cards, cap, want)
    # twice the rotation in one batch: the second sees the row the first left
    gen = _upload(ctx, n_cards, cap, used)
    rot = rows[5].astype(np.int32)
    ctx.gas_nodes_update(gen, gen + 1, [5, 5], [n_cards[5]] * 2, cap[[5, 5]], np.stack([rot, rot]))
    want = used.copy()
    want[5] = used[5][(np.arange(k) + 2) % k]
    _check_state(ctx, gen + 1, n_cards, cap, want)


# ------------------------------------------------------------------ 3. stale derived data

@pytest.mark.parametrize("k,q", SHAPES)
def test_fit_update_fit_sees_the_update(ctx, oracle, k, q):
    n_cards, cap, used = snapshot_for(k, q, 17 * k)
    a, b = 7, 100
    n_cards[[a, b]] = k
    used[a] = cap[a]  # full: nothing fits on a
    used[a, :, 0] = cap[a, 0]
    gen = _upload(ctx, n_cards, cap, used)
    before = _check_fit(ctx, oracle, gen, n_cards, cap, used)  # derived data is built
    n_before = int((before[:, a] >> 31).sum())  # (a pod without an i915 request selects nothing)
    ident = np.arange(k, dtype=np.int32)
    upd = (np.array([a, b], np.int32), np.array([k, k - 1], np.int32),
           np.stack([cap[a] * 4, cap[b]]), np.stack([ident, ident]))
    w_nc, w_cap, w_used, _ = replay(n_cards, cap, used, *upd)
    ctx.gas_nodes_update(gen, gen + 1, *upd)
    after = _check_fit(ctx, oracle, gen + 1, w_nc, w_cap, w_used)  # no call in between
    assert int((after[:, a] >> 31).sum()) > n_before
    # bind and place on the updated node
    req, mask, ncont = pods_for(q)
    pods = np.arange(6, dtype=np.int32)
    nodes = np.full(6, a, np.int32)
    res, st = ctx.gas_bind(gen + 1, gen + 2, pods, nodes, req, mask, ncont, 0)
    w_used, w_res, w_st = oracle.gas_bind(w_nc, w_cap, w_used, req, mask, ncont, 0, pods, nodes)
    np.testing.assert_array_equal(st, w_st)
    np.testing.assert_array_equal(res, w_res)
    assert (st == OK).any()
    cand = np.full((P, 1), a, np.int32)
    node, rank, res, n_placed = ctx.gas_place(gen + 2, gen + 3, req, mask, ncont, 0, cand)
    w_used, w_res, w_st = oracle.gas_bind(w_nc, w_cap, w_used, req, mask, ncont, 0,
                                          np.arange(P, dtype=np.int32), cand[:, 0])
    np.testing.assert_array_equal(node, np.where(w_st == OK, a, -1))
    np.testing.assert_array_equal(res, np.where(w_st == OK, w_res, 0))
    assert n_placed == int((w_st == OK).sum())
    _check_state(ctx, gen + 3, w_nc, w_cap, w_used)


# ------------------------------------------------------------------ 4. parked slots are inert

def _events(n_cards, k, q, seed):
    """Pod events with ranks inside each node's label, and a few ranks of parked slots."""
    rng = np.random.default_rng(seed)
    _, _, ncont = pods_for(q)
    e = 200
    kinds = (rng.random(e) < 0.4).astype(np.int32)
    pods = rng.integers(0, P, size=e).astype(np.int32)
    nodes = rng.integers(0, N, size=e).astype(np.int32)
    cpc = rng.integers(0, 3, size=(e, C)).astype(np.int32)
    cards = np.zeros((e, 6), np.int32)
    for i in range(e):
        nc = max(int(n_cards[nodes[i]]), 1)
        cards[i] = rng.integers(0, nc, size=6)
        if rng.random() < 0.2:
            cards[i, rng.integers(0, 6)] = min(nc, k - 1)  # a parked slot (or the last card)
    return kinds, pods, nodes, cpc, cards


def _run_sequence(ctx, n_cards, cap, used):
    k, q = used.shape[1:]
    req, mask, ncont = pods_for(q)
    gen = _upload(ctx, n_cards, cap, used)
    out = [ctx.gas_fit(gen, req, mask, ncont, 0)]
    rng = np.random.default_rng(5)
    pods = rng.integers(0, P, size=60).astype(np.int32)
    nodes = rng.integers(0, N, size=60).astype(np.int32)
    out += list(ctx.gas_bind(gen, gen + 1, pods, nodes, req, mask, ncont, 0))
    kinds, epods, enodes, cpc, cards = _events(n_cards, k, q, 6)
    ereq, emask = np.abs(req[epods]), mask[epods]
    out.append(ctx.gas_apply(gen + 1, gen + 2, kinds, np.arange(len(kinds)), enodes, ereq, emask,
                             ncont[epods], cpc, cards))
    out.append(ctx.gas_fit(gen + 2, req, mask, ncont, 0))
    return out, ctx.gas_snapshot_get()[1]


@pytest.mark.parametrize("k,q", SHAPES)
def test_parked_slots_are_inert(ctx, k, q):
    n_cards, cap, used = snapshot_for(k, q, 19 * k)
    parked = np.arange(k)[None, :] >= np.maximum(n_cards, 0)[:, None]  # [N][K]
    assert used[parked].any()
    zeroed = used.copy()
    zeroed[parked] = 0
    out_a, used_a = _run_sequence(ctx, n_cards, cap, used)
    out_b, used_b = _run_sequence(ctx, n_cards, cap, zeroed)
    for x, y in zip(out_a, out_b):
        np.testing.assert_array_equal(x, y)
    assert (out_a[2] == OK).any() and (out_a[3] == OK).any() and (out_a[3] == ERR_INPUT).any()
    np.testing.assert_array_equal(used_a[~parked], used_b[~parked])
    np.testing.assert_array_equal(used_a[parked], used[parked])  # the parked values stay
    assert not used_b[parked].any()
    assert (used_a[~parked] != used[~parked]).any()  # while the label cards' usage moved


# ------------------------------------------------------------------ 5. label flap

def _flap(k):
    """Card 1 of a 4-card node leaves the label and returns: (count, src) per step."""
    leave = np.full(k, -1, np.int32)
    leave[:4] = [0, 2, 3, 1]  # card1 parked behind the label cards
    back = np.full(k, -1, np.int32)
    back[:4] = [0, 3, 1, 2]   # and back at its rank
    return (3, leave), (4, back)


@pytest.mark.parametrize("k,q", SHAPES)
def test_label_flap_and_node_delete_keep_the_usage(ctx, oracle, k, q):
    n_cards, cap, used = snapshot_for(k, q, 23 * k)
    node = 33
    n_cards[node] = 4
    used[node, 4:] = 0
    (nc1, src1), (nc2, src2) = _flap(k)
    mid_used = used.copy()
    mid_used[node, :4] = used[node, [0, 2, 3, 1]]
    mid_nc = n_cards.copy()
    mid_nc[node] = 3
    # two calls: the model in between is the node with three cards
    gen = _upload(ctx, n_cards, cap, used)
    ctx.gas_nodes_update(gen, gen + 1, [node], [nc1], cap[[node]], src1[None])
    _check_state(ctx, gen + 1, mid_nc, cap, mid_used)
    model = mid_used.copy()
    model[node, 3] = 0  # what a snapshot built from the model holds: label cards only
    np.testing.assert_array_equal(_check_fit(ctx, oracle, gen + 1, mid_nc, cap, mid_used),
                                  oracle.gas_fit(mid_nc, cap, model, *pods_for(q), 0))
    ctx.gas_nodes_update(gen + 1, gen + 2, [node], [nc2], cap[[node]], src2[None])
    _check_state(ctx, gen + 2, n_cards, cap, used)
    _check_fit(ctx, oracle, gen + 2, n_cards, cap, used)
    # one batch with both updates
    gen = _upload(ctx, n_cards, cap, used)
    st = ctx.gas_nodes_update(gen, gen + 1, [node, node], [nc1, nc2], cap[[node, node]],
                              np.stack([src1, src2]))
    assert not st.any()
    _check_state(ctx, gen + 1, n_cards, cap, used)
    _check_fit(ctx, oracle, gen + 1, n_cards, cap, used)
    # the node leaves the lister (identity src) and returns
    ident = np.arange(k, dtype=np.int32)
    gone_nc, gone_cap = n_cards.copy(), cap.copy()
    gone_nc[node], gone_cap[node] = -1, 0
    ctx.gas_nodes_update(gen + 1, gen + 2, [node], [-1], np.zeros((1, q), np.int64), ident[None])
    _check_state(ctx, gen + 2, gone_nc, gone_cap, used)
    words = _check_fit(ctx, oracle, gen + 2, gone_nc, gone_cap, used)
    assert not (words[:, node] >> 31).any()
    ctx.gas_nodes_update(gen + 2, gen + 3, [node], [4], cap[[node]], ident[None])
    _check_state(ctx, gen + 3, n_cards, cap, used)
    _check_fit(ctx, oracle, gen + 3, n_cards, cap, used)


# ------------------------------------------------------------------ 6. malformed device arrays

@pytest.mark.parametrize("k,q", SHAPES)
def test_device_form_reads_malformed_arrays_defensively(ctx, k, q):
    n_cards, cap, used = snapshot_for(k, q, 29 * k)
    ident = np.arange(k, dtype=np.int32)
    far, low, twice = ident.copy(), ident.copy(), ident.copy()
    far[1] = 1000
    low[2] = I32_MIN
    twice[3] = 0  # slot 0 copied twice: a caller bug, inside the row
    nodes = np.array([-1, N, 3, 4, 10, 11, 12, 2**31 - 1], np.int32)
    ncs = np.array([1, 1, -2, k + 1, 2, 2, 2, 0], np.int32)
    caps = np.full((8, q), 9, np.int64)
    src = np.stack([ident, ident, ident, ident, far, low, twice, ident])
    gen = _upload(ctx, n_cards, cap, used)
    st = _update_device(ctx, gen, nodes, ncs, caps, src)
    np.testing.assert_array_equal(st, [ERR_INPUT] * 4 + [OK] * 3 + [ERR_INPUT])
    w_nc, w_cap, w_used = n_cards.copy(), cap.copy(), used.copy()
    for node in (10, 11, 12):
        w_nc[node], w_cap[node] = 2, 9
    w_used[10, 1] = 0
    w_used[11, 2] = 0
    w_used[12, 3] = used[12, 0]
    # every other row, count and capacity is bit-identical
    _check_state(ctx, gen + 1, w_nc, w_cap, w_used)
    np.testing.assert_array_equal(st, replay(n_cards, cap, used, nodes, ncs, caps, src)[3])


# ------------------------------------------------------------------ 7. generations, EINVAL

def test_generations_and_host_validation(ctx):
    k, q = 8, 3
    n_cards, cap, used = snapshot_for(k, q, 31)
    ident = np.arange(k, dtype=np.int32)
    gen = _upload(ctx, n_cards, cap, used)
    good = (np.array([3], np.int32), np.array([2], np.int32), cap[[3]], ident[None])

    def fails(code, gen_from, nodes, ncs, caps, src):
        with pytest.raises(pas_amd.PasError) as e:
            ctx.gas_nodes_update(gen_from, gen_from + 1, nodes, ncs, caps, src)
        assert e.value.code == code
        _check_state(ctx, gen, n_cards, cap, used)  # nothing changed, the generation stays

    fails(_lib.PAS_ESTALE, gen + 5, *good)
    with pytest.raises(pas_amd.PasError) as e:
        _update_device(ctx, gen + 5, *good)
    assert e.value.code == _lib.PAS_ESTALE
    with pytest.raises(pas_amd.PasError) as e:
        ctx.gas_snapshot_resize(gen + 5, gen + 6, N + 1, k)
    assert e.value.code == _lib.PAS_ESTALE
    _check_state(ctx, gen, n_cards, cap, used)
    fails(_lib.PAS_EINVAL, gen, [-1], *good[1:])
    fails(_lib.PAS_EINVAL, gen, [N], *good[1:])
    fails(_lib.PAS_EINVAL, gen, [3], [-2], *good[2:])
    fails(_lib.PAS_EINVAL, gen, [3], [k + 1], *good[2:])
    bad = ident.copy()
    bad[0] = k
    fails(_lib.PAS_EINVAL, gen, *good[:3], bad[None])
    bad = ident.copy()
    bad[5] = 4  # slot 4 twice
    fails(_lib.PAS_EINVAL, gen, *good[:3], bad[None])
    # negative values may repeat; the generation moves on success, also for an empty batch
    holes = np.full(k, -1, np.int32)
    assert list(ctx.gas_nodes_update(gen, gen + 1, [3], [2], cap[[3]], holes[None])) == [OK]
    assert ctx.gas_snapshot_info()[0] == gen + 1
    ctx.gas_nodes_update(gen + 1, gen + 7, np.zeros(0, np.int32), np.zeros(0, np.int32),
                         np.zeros((0, q), np.int64), np.zeros((0, k), np.int32))
    assert ctx.gas_snapshot_info()[0] == gen + 7


# ------------------------------------------------------------------ 8. resize

def test_resize_keeps_the_content_and_everything_works_after_it(ctx, oracle):
    import torch
    k, q, n2, k2 = 8, 3, 200, 16
    n_cards, cap, used = snapshot_for(k, q, 37)
    gen = _upload(ctx, n_cards, cap, used)
    req, mask, ncont = pods_for(q)
    ctx.gas_fit(gen, req, mask, ncont, 0)  # derived data of the old shape exists
    # a TAS snapshot of the old node count
    ctx.tas_snapshot_set(gen, np.zeros((1, N), np.int64), np.zeros((1, (N + 63) // 64), np.uint64))
    for bad in ((N - 1, k), (N, k - 1), (n2, 4)):
        with pytest.raises(pas_amd.PasError) as e:
            ctx.gas_snapshot_resize(gen, gen + 1, *bad)
        assert e.value.code == _lib.PAS_EINVAL
    assert ctx.gas_shape == (N, k, q)
    ctx.gas_snapshot_resize(gen, gen + 1, n2, k2, stream=torch.cuda.current_stream())
    assert ctx.gas_shape == (n2, k2, q) and ctx.gas_snapshot_info() == (gen + 1, n2, k2, q)
    w_nc = np.concatenate([n_cards, np.full(n2 - N, -1, np.int32)])
    w_cap = np.concatenate([cap, np.zeros((n2 - N, q), np.int64)])
    w_used = np.zeros((n2, k2, q), np.int64)
    w_used[:N, :k] = used
    _check_state(ctx, gen + 1, w_nc, w_cap, w_used)
    words = _check_fit(ctx, oracle, gen + 1, w_nc, w_cap, w_used)
    assert words.shape == (P, n2) and not (words[:, N:] >> 31).any()
    # a spare slot becomes a real node with more cards than the old pitch held
    upd = (np.array([150], np.int32), np.array([12], np.int32),
           np.array([[4, 3000, 3000]], np.int64), np.full((1, k2), -1, np.int32))
    w_nc, w_cap, w_used, _ = replay(w_nc, w_cap, w_used, *upd)
    assert list(ctx.gas_nodes_update(gen + 1, gen + 2, *upd)) == [OK]
    words = _check_fit(ctx, oracle, gen + 2, w_nc, w_cap, w_used)
    assert (words[:, 150] >> 31).any()
    # bind, apply and place after it
    pods = np.arange(8, dtype=np.int32)
    nodes = np.array([150, 150, 0, 3, 150, 199, 64, 150], np.int32)
    res, st = ctx.gas_bind(gen + 2, gen + 3, pods, nodes, req, mask, ncont, 0)
    w_used, w_res, w_st = oracle.gas_bind(w_nc, w_cap, w_used, req, mask, ncont, 0, pods, nodes)
    np.testing.assert_array_equal(st, w_st)
    np.testing.assert_array_equal(res, w_res)
    one = np.zeros((1, C, q), np.int64)
    one[0, 0] = [1, 100, 50]
    st = ctx.gas_apply(gen + 3, gen + 4, [ADD, ADD, REMOVE], [0, 0, 0], [150, 199, 150], one,
                       np.array([[7, 0, 0]], np.uint32), np.array([1], np.int32),
                       np.array([[1, 0, 0]] * 3, np.int32), np.array([[11], [0], [11]], np.int32))
    np.testing.assert_array_equal(st, [OK, OK, OK])  # (199 lists no card: the ADD is skipped)
    cand = np.tile(np.array([[199, 150]], np.int32), (P, 1))
    node, rank, res, n_placed = ctx.gas_place(gen + 4, gen + 5, req, mask, ncont, 0, cand)
    w_used, w_res, w_st = oracle.gas_bind(w_nc, w_cap, w_used, req, mask, ncont, 0,
                                          np.arange(P, dtype=np.int32), cand[:, 1])
    np.testing.assert_array_equal(node, np.where(w_st == OK, 150, -1))
    np.testing.assert_array_equal(rank, np.where(w_st == OK, 1, -1))
    _check_state(ctx, gen + 5, w_nc, w_cap, w_used)
    # the combined TAS + GAS top-k still needs equal node counts
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_gas_topk_device(gen, gen + 5, 1, 0, None, None, None, None, C, 0, None, None,
                                None, 4, 0, None, None, None)
    assert e.value.code == _lib.PAS_EINVAL and "node count" in str(e.value)
    # growing one dimension only, and a same-size call that only moves the generation
    ctx.gas_snapshot_resize(gen + 5, gen + 6, n2 + 1, k2)
    ctx.gas_snapshot_resize(gen + 6, gen + 7, n2 + 1, k2)
    w_nc = np.concatenate([w_nc, [-1]]).astype(np.int32)
    w_cap = np.concatenate([w_cap, np.zeros((1, q), np.int64)])
    w_used = np.concatenate([w_used, np.zeros((1, k2, q), np.int64)])
    _check_state(ctx, gen + 7, w_nc, w_cap, w_used)
    _check_fit(ctx, oracle, gen + 7, w_nc, w_cap, w_used)
