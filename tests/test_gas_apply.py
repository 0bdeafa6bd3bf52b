"""Pod events on the resident GAS usage (pas_gas_apply / pas_gas_apply_device): the reference
cache's adjustPodResources(add / remove) straight from a pod's annotation
(node_resource_cache.go:190-287, Cache.handlePod :493-538).

The ADD reference is the loop below, built from the oracle's or_rm_divide / or_rm_add_rm
(resourceMap.divide / addRM) and following checkPodResourceAdjustment line for line; label
cards hold every kind.  REMOVE is the oracle's gas_release.  Inputs keep the reference's answer
independent of Go-map order: no event has a negative amount and an overflow on one card.
Shapes: N = 130 nodes, Q = 3, C = 3, K in {8, 9, 17} (the three KMAX instantiations).  The
commit kernel runs workgroups of 1 024 sorted positions: the 1 000-event batches are one
partial workgroup, the 2 500-event batch three (the last one partial) with run heads in each,
and the 6 000 events on two nodes are runs that cross workgroups."""
import ctypes
import functools

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib

N, Q, C = 130, 3, 3
KS = [8, 9, 17]
ADD, REMOVE = _lib.PAS_GAS_EV_ADD, _lib.PAS_GAS_EV_REMOVE
OK, WONT_FIT, ERR_INPUT, ERR_OVERFLOW = (_lib.PAS_GAS_OK, _lib.PAS_GAS_WONT_FIT,
                                         _lib.PAS_GAS_ERR_INPUT, _lib.PAS_GAS_ERR_OVERFLOW)
UNK = _lib.PAS_REQ_UNKNOWN_KIND
I64_MAX = np.iinfo(np.int64).max
KEYS = [f"kind{q}" for q in range(Q)]


# ------------------------------------------------------------------ the reference loop

def ref_add(oracle, used_n, ncard, extra, req_p, mask_p, ncont, cpc_e, cards_e):
    """adjustPodResources(add) of one pod on one node: status, and used_n [K][Q] advanced on
    success.  `extra` holds the resourceMaps the reference creates for cards outside the
    label ({rank: or_rm}); no fit reads them."""
    lib = oracle.load()
    ncard = max(int(ncard), 0)
    # nodeRes := c.newCopyNodeStatus(nodeName)                                  (:199)
    node_res = {k: oracle.rm({KEYS[q]: int(used_n[k, q]) for q in range(Q)}, KEYS)
                for k in range(ncard)}
    for k, m in extra.items():
        node_res[k] = oracle.rm(oracle.rm_dict(m, KEYS), KEYS)
    off = 0
    for i in range(int(ncont)):                                               # (:203)
        num_cards = int(cpc_e[i])
        card_names = [int(k) for k in cards_e[off:off + num_cards]]           # (:205-206)
        off += num_cards
        if num_cards > 0:                                                      # (:208)
            request = oracle.rm({KEYS[q]: int(req_p[i, q]) for q in range(Q)
                                 if (int(mask_p[i]) >> q) & 1}, KEYS)          # (:209)
            lib.or_rm_divide(ctypes.byref(request), num_cards)                 # (:210)
            for name in card_names:                                            # (:212)
                key = name if 0 <= name < ncard else ("outside", name)
                if key not in node_res:                                        # (:213-216)
                    node_res[key] = oracle.OrRm()
                err = lib.or_rm_add_rm(ctypes.byref(node_res[key]), ctypes.byref(request))
                if err:                                                        # (:224-226)
                    return ERR_OVERFLOW if err == 2 else ERR_INPUT
    # checked: adjustPodResources repeats the same adds on the cache          (:249-276)
    for key, m in node_res.items():
        if isinstance(key, tuple):
            extra[key] = m
        else:
            for q in range(Q):
                used_n[key, q] = m.val[q]
    return OK


def ref_apply(oracle, n_cards, used, kinds, pods, nodes, req, mask, ncont, cpc, cards):
    """The events in call order: (used after, statuses)."""
    used = np.array(used, np.int64, copy=True)
    st = np.zeros(len(kinds), np.int32)
    extra = {}
    e = 0
    while e < len(kinds):
        p, n = int(pods[e]), int(nodes[e])
        if kinds[e] == ADD:
            st[e] = ref_add(oracle, used[n], n_cards[n], extra.setdefault(n, {}), req[p],
                            mask[p] & ~np.uint32(UNK), ncont[p], cpc[e], cards[e])
            e += 1
            continue
        f = e  # a run of REMOVE events: the oracle applies them in order
        while f < len(kinds) and kinds[f] == REMOVE:
            f += 1
        used, st[e:f] = oracle.gas_release(n_cards, used, req, mask, ncont, pods[e:f],
                                           nodes[e:f], cpc[e:f], cards[e:f])
        e = f
    return used, st


# ------------------------------------------------------------------ inputs

def snapshot_for(k, seed):
    rng = np.random.default_rng(seed)
    n_cards = rng.integers(1, k + 1, size=N).astype(np.int32)
    n_cards[0] = k  # a node with every card of the snapshot
    cap = rng.integers(500, 5000, size=(N, Q)).astype(np.int64)
    used = rng.integers(0, 400, size=(N, k, Q)).astype(np.int64)
    return n_cards, cap, used


@functools.lru_cache(maxsize=None)
def random_case(k, n_ev=1000, n_live=40):
    """About 1 000 mixed events over about 40 distinct nodes, with its reference answer."""
    import oracle
    rng = np.random.default_rng(1000 + k + n_ev)
    n_cards, cap, used = snapshot_for(k, 7 * k)
    live = rng.choice(N, size=n_live, replace=False)
    n_cards[live[0]] = 0    # a node without the cards label
    n_cards[live[1]] = -1   # a node the lister does not know
    hot = live[2:5]         # usage near INT64_MAX: adds overflow there
    n_cards[hot] = k
    used[hot, 0, 0] = I64_MAX - 500
    used[hot, k - 1, 2] = I64_MAX - 3
    n_pods = 64
    req = rng.integers(0, 1000, size=(n_pods, C, Q)).astype(np.int64)
    req[rng.random((n_pods, C, Q)) < 0.1] = 0
    mask = rng.integers(0, 1 << Q, size=(n_pods, C)).astype(np.uint32)
    ncont = rng.integers(0, C + 1, size=n_pods).astype(np.int32)
    negative = np.arange(n_pods) % 8 == 7   # pods with a negative amount: never on a hot node
    for p in np.nonzero(negative)[0]:
        req[p, rng.integers(0, C), rng.integers(0, Q)] = -int(rng.integers(1, 50))
    mask[np.arange(n_pods) % 16 == 3, 0] |= np.uint32(UNK)  # ADD ignores it, REMOVE does not
    ld = 12
    kinds = (rng.random(n_ev) < 0.4).astype(np.int32)  # 1 = REMOVE
    pods = rng.integers(0, n_pods, size=n_ev).astype(np.int32)
    nodes = rng.choice(live, size=n_ev).astype(np.int32)
    on_hot = np.isin(nodes, hot) & negative[pods]
    pods[on_hot] -= 1  # the pod before a negative one is not negative
    cpc = rng.integers(0, 5, size=(n_ev, C)).astype(np.int32)  # sums stay within ld = 12
    cards = np.full((n_ev, ld), -1, np.int32)
    for e in range(n_ev):
        nc = max(int(n_cards[nodes[e]]), 1)
        row = rng.integers(0, nc, size=ld)  # small ranges: cards are listed repeatedly
        out = rng.random(ld) < 0.03
        row[out] = rng.choice([-1, nc, k, k + 3, 2**31 - 1, -2**31], size=int(out.sum()))
        cards[e] = row
    want_used, want_st = ref_apply(oracle, n_cards, used, kinds, pods, nodes, req, mask, ncont,
                                   cpc, cards)
    case = dict(n_cards=n_cards, cap=cap, used=used, kinds=kinds, pods=pods, nodes=nodes,
                req=req, mask=mask, ncont=ncont, cpc=cpc, cards=cards, want_used=want_used,
                want_st=want_st)
    for a in case.values():
        a.setflags(write=False)
    return case


_gen = [52000]


def _upload(ctx, n_cards, cap, used):
    _gen[0] += 10
    ctx.gas_snapshot_set(_gen[0], n_cards, cap, used)
    return _gen[0]


def _apply(ctx, gen, i):
    return ctx.gas_apply(gen, gen + 1, i["kinds"], i["pods"], i["nodes"], i["req"], i["mask"],
                         i["ncont"], i["cpc"], i["cards"])


def _dev(a):
    import torch
    a = np.array(a)  # (a copy: the shared inputs are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _apply_device(ctx, gen, kinds, pods, nodes, req, mask, ncont, cpc, cards, n_pods=None):
    import torch
    e = len(kinds)
    st_t = torch.full((e,), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    ctx.gas_apply_device(gen, gen + 1, e, _dev(kinds), _dev(pods), _dev(nodes),
                         req.shape[0] if n_pods is None else n_pods, req.shape[1], _dev(req),
                         _dev(mask), _dev(ncont), _dev(cpc), _dev(cards), cards.shape[1], st_t,
                         stream=stream)
    stream.synchronize()
    return st_t.cpu().numpy()


# ------------------------------------------------------------------ CPU: the reference loop

def test_reference_loop_small_cases(oracle):
    # 10 / 3 truncates; a card listed twice is added to twice; a card outside the label
    # counts towards numCards; a negative amount is errInput and nothing changes
    n_cards = np.array([2], np.int32)
    used = np.array([[[1, 5], [0, 0], [9, 9]]], np.int64)  # K = 3, 2 label cards
    req = np.zeros((2, C, Q), np.int64)
    req[0, 0, :2] = [10, 7]
    req[1, 0, :2] = [4, -3]
    mask = np.zeros((2, C), np.uint32)
    mask[:, 0] = 3
    ncont = np.ones(2, np.int32)
    cpc = np.array([[3, 0, 0], [1, 0, 0]], np.int32)
    cards = np.array([[0, 0, 2, -1], [1, -1, -1, -1]], np.int32)
    pad = np.zeros((1, 3, Q), np.int64)
    pad[:, :, :2] = used
    after, st = ref_apply(oracle, n_cards, pad, [ADD, ADD], [0, 1], [0, 0], req, mask, ncont,
                          cpc, cards)
    assert list(st) == [OK, ERR_INPUT]
    np.testing.assert_array_equal(after[0, :, :2], [[1 + 3 + 3, 5 + 2 + 2], [0, 0], [9, 9]])


# ------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_random_batch_parity(ctx, k):
    i = random_case(k)
    assert len(np.unique(i["nodes"])) >= 35
    for s in (OK, ERR_INPUT, ERR_OVERFLOW):  # the batch reaches every status
        assert (i["want_st"] == s).any()
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])
    st = _apply(ctx, gen, i)
    g, after = ctx.gas_snapshot_get()
    assert g == gen + 1
    np.testing.assert_array_equal(st, i["want_st"])
    np.testing.assert_array_equal(after, i["want_used"])


@pytest.mark.gpu
def test_random_batch_three_workgroups(ctx):
    i = random_case(8, 2500, N)  # every node has a run; heads in all three workgroups
    assert len(np.unique(i["nodes"])) == N
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])
    st = _apply(ctx, gen, i)
    np.testing.assert_array_equal(st, i["want_st"])
    np.testing.assert_array_equal(ctx.gas_snapshot_get()[1], i["want_used"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_adopt_equals_bind(ctx, oracle, k):
    from test_gas_gpu import random_gas
    rng = np.random.default_rng(300 + k)
    n_cards, cap, used, req, mask, ncont = random_gas(rng, N, k, Q, 80, C, False, 0)
    pods = rng.integers(0, 80, size=300).astype(np.int32)
    nodes = rng.integers(0, N, size=300).astype(np.int32)
    gen = _upload(ctx, n_cards, cap, used)
    res, st, sel, nsel = ctx.gas_bind(gen, gen + 1, pods, nodes, req, mask, ncont, 0,
                                      selections=True)
    _, bound = ctx.gas_snapshot_get()
    ok = np.nonzero((st == OK) & (nsel >= 0))[0]
    assert len(ok) > 50 and (nsel[ok] > 0).any()
    # the annotations the binds returned: container c takes its numI915 selections, in order
    cpc = np.zeros((len(ok), C), np.int32)
    for j, b in enumerate(ok):
        p = pods[b]
        for c in range(ncont[p]):
            if (mask[p, c] >> 0) & 1 and req[p, c, 0] > 0:
                cpc[j, c] = req[p, c, 0]
        assert cpc[j].sum() == nsel[b]
    cards = sel[ok].astype(np.int32)  # [B][64], ranks
    # the binds that fit, adopted on a fresh upload of the same snapshot
    gen = _upload(ctx, n_cards, cap, used)
    st2 = ctx.gas_apply(gen, gen + 1, np.full(len(ok), ADD, np.int32), pods[ok], nodes[ok], req,
                        mask, ncont, cpc, cards)
    assert (st2 == OK).all()
    _, adopted = ctx.gas_snapshot_get()
    want, _, w_st = oracle.gas_bind(n_cards, cap, used, req, mask, ncont, 0, pods[ok], nodes[ok])
    assert (w_st == OK).all()
    np.testing.assert_array_equal(adopted, want)
    np.testing.assert_array_equal(adopted, bound)  # a bind that does not fit changes nothing
    # REMOVE them all: back to the snapshot (no kind clamps: every subtraction undoes an add)
    st3 = ctx.gas_apply(gen + 1, gen + 2, np.full(len(ok), REMOVE, np.int32), pods[ok],
                        nodes[ok], req, mask, ncont, cpc, cards)
    assert (st3 == OK).all()
    _, back = ctx.gas_snapshot_get()
    np.testing.assert_array_equal(back, used)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_atomicity_and_statuses(ctx, oracle, k):
    n_cards, cap, used = snapshot_for(k, 11 * k)
    n_cards[:4] = k
    used[:4] = 5
    used[1, k - 1, 1] = I64_MAX - 10
    cap[3] = 100
    req = np.zeros((4, C, Q), np.int64)
    mask = np.zeros((4, C), np.uint32)
    ncont = np.array([2, 2, 1, 1], np.int32)
    req[0, 0], mask[0, 0] = [7, 8, 9], 7      # pod 0: container 0 valid,
    req[0, 1], mask[0, 1] = [1, 22, 3], 7     #        container 1 overflows kind 1 (2 cards)
    req[1, 0], mask[1, 0] = [7, 8, 9], 7      # pod 1: container 0 valid,
    req[1, 1], mask[1, 1] = [4, -2, 4], 2     #        container 1 has a negative amount
    req[2, 0], mask[2, 0] = [4, -2, 4], 5     # pod 2: the negative kind is not in the mask
    req[3, 0], mask[3, 0] = [1000, 0, 0], 1   # pod 3: far above node 3's capacity of 100
    kinds = np.full(5, ADD, np.int32)
    pods = np.array([0, 0, 1, 2, 3], np.int32)
    nodes = np.array([1, 0, 2, 2, 3], np.int32)
    cpc = np.zeros((5, C), np.int32)
    cards = np.full((5, 4), -1, np.int32)
    cpc[0, :2], cards[0] = [2, 2], [0, 1, 0, k - 1]   # node 1: card k-1 holds INT64_MAX - 10
    cpc[1, :2], cards[1] = [2, 2], [0, 1, 0, k - 1]   # node 0: the same pod fits
    cpc[2, :2], cards[2, :3] = [2, 1], [0, 1, 2]
    cpc[3, 0], cards[3, :1] = 1, [2]
    cpc[4, 0], cards[4, :1] = 1, [0]
    gen = _upload(ctx, n_cards, cap, used)
    st = ctx.gas_apply(gen, gen + 1, kinds, pods, nodes, req, mask, ncont, cpc, cards)
    want_used, want_st = ref_apply(oracle, n_cards, used, kinds, pods, nodes, req, mask, ncont,
                                   cpc, cards)
    assert list(want_st) == [ERR_OVERFLOW, OK, ERR_INPUT, OK, OK]
    np.testing.assert_array_equal(st, want_st)
    _, after = ctx.gas_snapshot_get()
    np.testing.assert_array_equal(after, want_used)
    np.testing.assert_array_equal(after[1], used[1])  # container 0's cards are unchanged
    np.testing.assert_array_equal(after[0, 0], [5 + 3 + 0, 5 + 4 + 11, 5 + 4 + 1])
    np.testing.assert_array_equal(after[2, 2], [5 + 4, 5, 5 + 4])
    assert after[3, 0, 0] == 1005 and after[3, 0, 0] > cap[3, 0]  # no capacity check
    # ... and the fit rejects a node whose usage is above its capacity
    one = np.zeros((1, C, Q), np.int64)
    one[0, 0, 0] = 1
    m1 = np.zeros((1, C), np.uint32)
    m1[0, 0] = 1
    n_cards3 = np.array(n_cards)
    fit_before = ctx.gas_fit(gen + 1, one, m1, np.ones(1, np.int32), 0)
    assert n_cards3[3] == k and k > 1 and (fit_before[0, 3] >> 31) == 1  # card 1 still takes it
    node3 = np.full(k, 3, np.int32)
    full = np.zeros((k, C), np.int32)
    full[:, 0] = 1
    st = ctx.gas_apply(gen + 1, gen + 2, np.full(k, ADD, np.int32), np.full(k, 3, np.int32),
                       node3, req, mask, ncont, full, np.arange(k, dtype=np.int32)[:, None])
    assert (st == OK).all()
    fit_after = ctx.gas_fit(gen + 2, one, m1, np.ones(1, np.int32), 0)
    assert (fit_after[0, 3] >> 31) == 0
    np.testing.assert_array_equal(np.delete(fit_after[0], 3), np.delete(fit_before[0], 3))


@pytest.mark.gpu
def test_order_within_a_node_across_sort_blocks(ctx, oracle):
    # 6 000 events on 2 nodes, alternating ADD and REMOVE of random amounts on one card from
    # 0: the clamp at 0 makes the result depend on the order
    k = 8
    rng = np.random.default_rng(77)
    n_cards, cap, used = snapshot_for(k, 5)
    two = np.array([17, 101])
    n_cards[two] = k
    used[two] = 0
    n_pods = 50
    req = np.zeros((n_pods, C, Q), np.int64)
    req[:, 0, :] = rng.integers(0, 1000, size=(n_pods, Q))
    mask = np.zeros((n_pods, C), np.uint32)
    mask[:, 0] = 7
    ncont = np.ones(n_pods, np.int32)
    n_ev = 6000
    kinds = (np.arange(n_ev) % 2).astype(np.int32)
    pods = rng.integers(0, n_pods, size=n_ev).astype(np.int32)
    nodes = two[rng.integers(0, 2, size=n_ev)].astype(np.int32)
    cpc = np.zeros((n_ev, C), np.int32)
    cpc[:, 0] = 1
    cards = np.full((n_ev, 1), 3, np.int32)
    want_used, want_st = ref_apply(oracle, n_cards, used, kinds, pods, nodes, req, mask, ncont,
                                   cpc, cards)
    assert (want_st == OK).all()
    # the order matters: the same events with the ADDs first end elsewhere
    order = np.argsort(kinds, kind="stable")
    other, _ = ref_apply(oracle, n_cards, used, kinds[order], pods[order], nodes[order], req,
                         mask, ncont, cpc[order], cards[order])
    assert (other[two] != want_used[two]).any()
    gen = _upload(ctx, n_cards, cap, used)
    st = ctx.gas_apply(gen, gen + 1, kinds, pods, nodes, req, mask, ncont, cpc, cards)
    np.testing.assert_array_equal(st, want_st)
    _, after = ctx.gas_snapshot_get()
    np.testing.assert_array_equal(after, want_used)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_host_and_device_forms_agree(ctx, k):
    i = random_case(k)
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])
    st_h = _apply(ctx, gen, i)
    _, used_h = ctx.gas_snapshot_get()
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])
    st_d = _apply_device(ctx, gen, i["kinds"], i["pods"], i["nodes"], i["req"], i["mask"],
                         i["ncont"], i["cpc"], i["cards"])
    g, used_d = ctx.gas_snapshot_get()
    assert g == gen + 1
    np.testing.assert_array_equal(st_d, st_h)
    np.testing.assert_array_equal(used_d, used_h)
    np.testing.assert_array_equal(st_d, i["want_st"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_device_form_malformed_inputs(ctx, oracle, k):
    # nothing here is meant to fault: the _device form clamps and skips
    n_cards, cap, used = snapshot_for(k, 13 * k)
    n_pods, ld = 6, 4
    req = np.zeros((n_pods, C, Q), np.int64)
    req[:, :, :] = np.arange(1, Q + 1) * 10
    mask = np.full((n_pods, C), 7, np.uint32)
    ncont = np.array([1, 2, C + 5, -3, 2**31 - 1, 3], np.int32)  # 2.. are out of range
    rows = [
        # kind, pod, node, cpc, cards
        (ADD, 0, 5, [1, 0, 0], [0, -1, -1, -1]),             # 0 valid
        (ADD, 0, -1, [1, 0, 0], [0, -1, -1, -1]),            # 1 node -1
        (ADD, 0, N, [1, 0, 0], [0, -1, -1, -1]),             # 2 node N
        (REMOVE, n_pods, 5, [1, 0, 0], [0, -1, -1, -1]),     # 3 pod n_pods
        (7, 0, 5, [1, 0, 0], [0, -1, -1, -1]),               # 4 kind 7
        (-1, 0, 5, [1, 0, 0], [0, -1, -1, -1]),              # 5 kind -1
        (ADD, 1, 6, [-4, 2, 0], [0, 0, -1, -1]),             # 6 a negative count reads as 0
        (ADD, 1, 6, [3, 2, 0], [0, 0, 0, 0]),                # 7 counts run past cards_ld
        (ADD, 1, 6, [2**31 - 1, 2**31 - 1, 0], [0, 0, 0, 0]),  # 8 ... far past it
        (REMOVE, 1, 6, [4, 1, 0], [0, 0, 0, 0]),             # 9 ... on REMOVE too
        (ADD, 2, 7, [1, 1, 2], [0, 0, 0, 0]),                # 10 n_containers C + 5 reads as C
        (ADD, 3, 7, [1, 1, 1], [0, 0, 0, -1]),               # 11 n_containers -3 reads as 0
        (ADD, 4, 7, [1, 1, 1], [0, 0, 0, -1]),               # 12 n_containers INT32_MAX: C
        (REMOVE, 5, 8, [1, 1, 1], [0, 0, 0, -1]),            # 13 valid
        (ADD, -2**31, 2**31 - 1, [1, 0, 0], [0, 0, 0, 0]),   # 14 pod and node far out
    ]
    kinds = np.array([r[0] for r in rows], np.int32)
    pods = np.array([r[1] for r in rows], np.int32)
    nodes = np.array([r[2] for r in rows], np.int32)
    cpc = np.array([r[3] for r in rows], np.int32)
    cards = np.array([r[4] for r in rows], np.int32)
    n_cards[5:9] = max(k // 2, 1)
    bad = [1, 2, 3, 4, 5, 7, 8, 9, 14]
    good = [e for e in range(len(rows)) if e not in bad]
    # what the valid events do, as the contract reads them
    ncont_read = np.clip(ncont.astype(np.int64), 0, C).astype(np.int32)
    want_used, want_st = ref_apply(oracle, n_cards, used, kinds[good], pods[good], nodes[good],
                                   req, mask, ncont_read, np.maximum(cpc[good], 0), cards[good])
    assert (want_st == OK).all()
    gen = _upload(ctx, n_cards, cap, used)
    st = _apply_device(ctx, gen, kinds, pods, nodes, req, mask, ncont, cpc, cards, n_pods)
    assert list(st[bad]) == [ERR_INPUT] * len(bad)
    np.testing.assert_array_equal(st[good], want_st)
    g, after = ctx.gas_snapshot_get()
    assert g == gen + 1
    np.testing.assert_array_equal(after, want_used)
    touched = np.zeros(N, bool)
    touched[[5, 6, 7, 8]] = True
    np.testing.assert_array_equal(after[~touched], used[~touched])
    # the host form refuses the same arrays before anything runs
    for e in bad + [6, 10, 11, 12]:
        with pytest.raises(pas_amd.PasError) as err:
            ctx.gas_apply(gen + 1, gen + 2, kinds[e:e + 1], pods[e:e + 1], nodes[e:e + 1], req,
                          mask, ncont, cpc[e:e + 1], cards[e:e + 1])
        assert err.value.code == _lib.PAS_EINVAL
    assert ctx.gas_snapshot_get()[0] == gen + 1


@pytest.mark.gpu
def test_generation(ctx):
    i = random_case(8)
    gen = _upload(ctx, i["n_cards"], i["cap"], i["used"])
    with pytest.raises(pas_amd.PasError) as err:
        _apply(ctx, gen - 1, i)
    assert err.value.code == _lib.PAS_ESTALE
    with pytest.raises(pas_amd.PasError) as err:
        _apply_device(ctx, gen + 1, i["kinds"], i["pods"], i["nodes"], i["req"], i["mask"],
                      i["ncont"], i["cpc"], i["cards"])
    assert err.value.code == _lib.PAS_ESTALE
    g, after = ctx.gas_snapshot_get()
    assert g == gen
    np.testing.assert_array_equal(after, i["used"])
    _apply(ctx, gen, i)
    assert ctx.gas_snapshot_get()[0] == gen + 1
    with pytest.raises(pas_amd.PasError) as err:  # the old generation is stale for the fit
        ctx.gas_fit(gen, i["req"], i["mask"] & ~np.uint32(UNK), i["ncont"], 0)
    assert err.value.code == _lib.PAS_ESTALE
    ctx.gas_fit(gen + 1, i["req"], i["mask"] & ~np.uint32(UNK), i["ncont"], 0)
    # an empty batch still moves the generation
    empty = np.zeros(0, np.int32)
    st = ctx.gas_apply(gen + 1, gen + 2, empty, empty, empty, i["req"], i["mask"], i["ncont"],
                       np.zeros((0, C), np.int32), np.zeros((0, 1), np.int32))
    assert len(st) == 0 and ctx.gas_snapshot_get()[0] == gen + 2
    with pytest.raises(pas_amd.PasError) as err:  # cards_ld < 1
        ctx.gas_apply(gen + 2, gen + 3, empty, empty, empty, i["req"], i["mask"], i["ncont"],
                      np.zeros((0, C), np.int32), np.zeros((0, 0), np.int32))
    assert err.value.code == _lib.PAS_EINVAL
