"""Resumed top-k lists (pas_tas_gas_topk_after_device, pas_tas_gas_topk_wide_after_device).

Definition (include/pas.h, "Resuming a top-k list"): the result for a pod is the list of the
entry point without _after with k unbounded, minus every record that is not strictly after the
pod's cursor in ascending (key[, sub], node), cut at k.  The restatement below says that over
an explicit list of records (Python tuples compare in exactly that order) and is checked
against brute force on the CPU; the GPU tests compare the device against it, with the existing
entry point at a large k as the list (itself pinned to the oracle by
test_tas_gas_topk_equals_composition / test_tas_gas_topk_wide_equals_composition)."""
import bisect
import ctypes
import functools

import numpy as np
import pytest
import torch

import pas_amd
from pas_amd import _lib
from pas_amd import workload as wl
from pas_amd.context import RULE_DTYPE
from pas_amd.shard import node_range
from pas_amd.workload import pack_bits
from test_shard import _dev, _rule_tensors, make_case, shard_cand, shard_snapshot

LT, GT, EQ = 0, 1, 2
I64_MIN, I64_MAX = -2**63, 2**63 - 1
I32_MAX, U32_MAX = 2**31 - 1, 2**32 - 1
AFTER_ARGS = _lib.SIGNATURES["pas_tas_gas_topk_after_device"][1]
WIDE_AFTER_ARGS = _lib.SIGNATURES["pas_tas_gas_topk_wide_after_device"][1]


# ------------------------------------------------------------------ the restatement
def restated_start(recs, cursor):
    """Number of records of the ascending list recs that are <= cursor."""
    return bisect.bisect_right(recs, cursor)


def resumed(recs, cursor, k):
    """The records strictly after cursor, cut at k."""
    s = restated_start(recs, cursor)
    return recs[s:s + k]


def test_restated_start_equals_brute_force():
    """Random rows with heavy ties (few distinct keys, hundreds of nodes each), 64-bit and wide
    records; cursors on records, between records, the sentinels and random bit patterns."""
    rng = np.random.default_rng(0xAF7E)
    for width in (2, 3):
        for _ in range(30):
            n = int(rng.integers(0, 400))
            keys = rng.choice(rng.integers(-4, 4, 5) * 2**60, n).tolist()
            subs = rng.choice([0, 1, 500_000_000, U32_MAX], n).tolist()
            nodes = rng.permutation(2000)[:n].tolist()
            recs = sorted(zip(keys, subs, nodes) if width == 3 else zip(keys, nodes))
            begin = (I64_MIN, 0, -1) if width == 3 else (I64_MIN, -1)
            end = (I64_MAX, U32_MAX, I32_MAX) if width == 3 else (I64_MAX, I32_MAX)
            cursors = [begin, end] + recs[::7]
            for _ in range(40):
                c = [int(rng.choice(keys + [0, 1, -1])) + int(rng.integers(-1, 2))]
                if width == 3:
                    c.append(int(rng.choice([0, 1, 499_999_999, U32_MAX])))
                c.append(int(rng.integers(-5, 2100)))
                cursors.append(tuple(c))
            for c in cursors:
                want = sum(1 for r in recs if r <= c)
                assert restated_start(recs, c) == want
                assert resumed(recs, c, 9) == [r for r in recs if r > c][:9]
            assert restated_start(recs, begin) == 0 and resumed(recs, end, 5) == []


# ------------------------------------------------------------------ binding (CPU)
def test_symbols_and_signatures():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "pas_tas_gas_topk_after_device")
    assert hasattr(lib, "pas_tas_gas_topk_wide_after_device")
    P, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    head = [P, u64, u64, i32, i32, P, P, P, P, i32, i32, P, P, P, i32, i32]
    # the arguments of the entry points without _after, the cursor arrays before the outputs
    assert _lib.SIGNATURES["pas_tas_gas_topk_device"][1] == head + [P] * 3 + [P]
    assert AFTER_ARGS == head + [P] * 2 + [P] * 3 + [P]
    assert _lib.SIGNATURES["pas_tas_gas_topk_wide_device"][1] == head + [P] * 4 + [P]
    assert WIDE_AFTER_ARGS == head + [P] * 3 + [P] * 4 + [P]
    assert pas_amd.LIB.pas_abi_version() == 3


def test_null_context():
    z = [None, 1, 2, 0, 0, None, None, None, None, 0, 0, None, None, None, 1, 0]
    assert pas_amd.LIB.pas_tas_gas_topk_after_device(*z, *[None] * 6) == _lib.PAS_EINVAL
    assert pas_amd.LIB.pas_tas_gas_topk_wide_after_device(*z, *[None] * 8) == _lib.PAS_EINVAL


# ------------------------------------------------------------------ the case
N, P, M = 3000, 96, 6
BASE = 1234


@functools.lru_cache(maxsize=None)
def paging_case(cards, cand_frac):
    """N = 3 000 nodes, 96 pods, 6 metrics; computed once per variant and never modified.
    Metric 0 has 8 distinct values and metric 1 has 5, so their tie runs span hundreds of nodes
    and every cursor of a pod prioritizing them falls inside one; three quarters of the pods
    prioritize one of the two.  Operators cycle GreaterThan, LessThan, Equals and an unknown
    one (index order).  Pods 0-3 carry dontschedule rules on their own prioritize metric
    (ranges the walk jumps over: at the head of the order, in its middle, two at once), pod 4
    has 40 rules (its wave takes the unstaged path), pods 5 and 6 prioritize a metric out of
    range (empty list), pods 7 and 8 fit nowhere."""
    from test_gas_gpu import random_gas
    snap, batch = make_case(0xAF7 + cards, N, M, P, 4, cand_frac=cand_frac)
    rng = np.random.default_rng(0xAF70 + cards)
    v = snap.v_milli.copy()
    v[0] = rng.integers(0, 8, N) * 1000
    v[1] = rng.integers(0, 5, N) * 1000
    per_pod = [[tuple(r) for r in batch.rules[batch.rule_off[p]:batch.rule_off[p + 1]]
                if r["metric"] > 1] for p in range(P)]  # (targets drawn for the old columns)
    prio = batch.prio.copy()
    prio["metric"] = np.where(np.arange(P) % 4 == 3, rng.integers(2, M, P), np.arange(P) % 2)
    prio["op"] = np.array([GT, LT, EQ, 7])[(np.arange(P) // 2) % 4]
    special = [((0, GT), [(0, GT, 5)]), ((0, LT), [(0, LT, 2)]), ((0, GT), [(0, EQ, 6)]),
               ((0, LT), [(0, EQ, 0), (0, GT, 6)]),
               ((0, LT), [(int(rng.integers(0, M)), LT, -10) for _ in range(39)] + [(0, EQ, 3)])]
    for p, (pr, rl) in enumerate(special):
        per_pod[p] = rl
        prio[p] = pr + (0,)
    prio["metric"][5], prio["metric"][6] = 99, M
    rules = np.array([r for rl in per_pod for r in rl], RULE_DTYPE)
    off = np.cumsum([0] + [len(rl) for rl in per_pod]).astype(np.int32)
    if cards == 8:
        gs, gb, i915 = wl.make_gas_snapshot(N, seed=0xAF7), wl.make_gas_batch(P, seed=0xAF7), 0
        # one GPU with more millicores than a card has
        gb.req[7:9, 0, :2], gb.req_mask[7:9, 0] = (1, 10**9), 0b111
    else:
        nc, cap, used, req, mask, ncont = random_gas(rng, N, cards, 3, P, 4, i915=0)
        cap *= 4
        req[7:9, 0, :2], mask[7:9, 0], ncont[7:9] = (1, 10**9), 0b111, 1
        gs, gb, i915 = wl.GasSnapshotData(nc, cap, used), wl.GasBatch(req, mask, ncont), 0
    out = dict(v=v, pres=snap.present, rules=rules, off=off, prio=prio, cand=batch.cand, gs=gs,
               gb=gb, i915=i915)
    for a in (v, rules, off, prio):
        a.setflags(write=False)
    return out


class Dev:
    """A case on the device: both snapshots set on ctx (nodes [n0, n1) of the case) and the
    batch tensors; topk() runs the 64-bit or the wide entry point, with or without cursors."""
    _gen = [52000]

    def __init__(self, ctx, c, n0=0, n1=None, scale=None, wide=None):
        from test_topk_wide import set_snapshot
        n = c["v"].shape[1]
        n1 = n if n1 is None else n1
        Dev._gen[0] += 10
        g = Dev._gen[0]
        sv, sp = shard_snapshot(c["v"], c["pres"], n0, n1)
        if scale is None:
            ctx.tas_snapshot_set(g, sv, sp)
            self.tas_gen = g
        else:
            self.tas_gen = set_snapshot(ctx, g, sv, sp, scale,
                                        {m: (w[n0:n1], f[n0:n1]) for m, (w, f) in wide.items()})
        gs, gb = c["gs"], c["gb"]
        self.gas_gen = g + 5
        ctx.gas_snapshot_set(self.gas_gen, gs.n_cards[n0:n1], gs.cap[n0:n1], gs.used[n0:n1])
        self.ctx, self.P, self.nr = ctx, len(c["prio"]), len(c["rules"])
        # (copies: the shared inputs are read-only)
        batch = wl.TasBatch(np.array(c["rules"]), np.array(c["off"]), np.array(c["prio"]))
        self.tas = _rule_tensors(batch, shard_cand(c["cand"], n, n0, n1))
        self.gas = (gb.req.shape[1], c["i915"], _dev(gb.req), _dev(gb.req_mask.view(np.int32)),
                    _dev(gb.n_containers))

    def topk(self, k, base, after=None, wide=False):
        """Records as numpy (key, [sub,] node, len); after = (key, [sub,] node) numpy arrays."""
        P = self.P
        key = torch.empty((P, k), dtype=torch.int64, device="cuda")
        sub = torch.empty((P, k), dtype=torch.int32, device="cuda")
        node = torch.empty((P, k), dtype=torch.int32, device="cuda")
        ln = torch.empty(P, dtype=torch.int32, device="cuda")
        head = (self.tas_gen, self.gas_gen, P, self.nr, *self.tas, *self.gas, k, base)
        outs = (key, sub, node, ln) if wide else (key, node, ln)
        if after is None:
            fn = self.ctx.tas_gas_topk_wide_device if wide else self.ctx.tas_gas_topk_device
            fn(*head, *outs)
        else:
            cur = [_dev(after[0].astype(np.int64))]
            if wide:
                cur.append(_dev(after[1].astype(np.uint32).view(np.int32)))
            cur.append(_dev(after[-1].astype(np.int32)))
            fn = (self.ctx.tas_gas_topk_wide_after_device if wide
                  else self.ctx.tas_gas_topk_after_device)
            fn(*head, *cur, *outs)
        self.ctx.synchronize()
        got = [key.cpu().numpy()]
        if wide:
            got.append(sub.cpu().numpy().view(np.uint32))
        return tuple(got + [node.cpu().numpy(), ln.cpu().numpy()])


def last_record(page, k):
    """The cursor a page hands to the next call: its last record, padding included."""
    return tuple(a[:, k - 1] for a in page[:-1])


def check_paging(dev, k, base, wide, min_paged=1 / 3):
    """Pages of k through the _after entry point against the existing entry point at K = 8 k:
    page i is records [i k, (i + 1) k) of the long list, padding and length included; the page
    after a short page is empty.  Returns the long list."""
    K = 8 * k
    full = dev.topk(K, base, wide=wide)
    L = full[-1]
    # (otherwise paging is never exercised)
    assert (L > 2 * k).mean() >= min_paged, (L > 2 * k).mean()
    cur = (np.full(dev.P, I64_MIN),) + ((np.zeros(dev.P, np.uint32),) if wide else ()) + \
        (np.full(dev.P, -1),)
    for i in range(9):
        page = dev.topk(k, base, after=cur, wide=wide)
        if i < 8:
            for got, want in zip(page[:-1], full[:-1]):  # key, [sub,] node
                np.testing.assert_array_equal(got, want[:, i * k:(i + 1) * k], f"page {i}")
            np.testing.assert_array_equal(page[-1], np.clip(L - i * k, 0, k), f"page {i} len")
        else:  # past the long list: only pods whose whole list it holds can be judged
            done = L < K
            assert (page[-1][done] == 0).all()
            assert (page[-2][done] == I32_MAX).all() and (page[0][done] == I64_MAX).all()
        cur = last_record(page, k)
    return full


# ------------------------------------------------------------------ 1. pages = the long list
@pytest.mark.gpu
@pytest.mark.parametrize("k,cards,cand_frac", [(1, 8, None), (7, 8, 0.8), (16, 12, None),
                                               (33, 8, None), (16, 8, 0.9)])
def test_resumed_pages_equal_long_list(ctx, k, cards, cand_frac):
    c = paging_case(cards, cand_frac)
    dev = Dev(ctx, c)
    key, node, L = check_paging(dev, k, BASE, wide=False)
    # the case holds what it claims: jumped pods with lists, the long pod, empty and unfit pods
    assert (L[:5] > 0).all() and c["off"][5] - c["off"][4] == 40
    assert L[5] == 0 and L[6] == 0 and L[7] == 0 and L[8] == 0
    ops = c["prio"]["op"][L > 2 * k]
    assert {GT, LT, EQ, 7} <= set(ops.tolist())


# ------------------------------------------------------------------ 2. sentinels, any cursor
def _full_lists(dev, base, wide=False):
    """Every pod's whole list as ascending tuples (k = the node count)."""
    full = dev.topk(N, base, wide=wide)
    L = full[-1]
    return [list(zip(*(a[p, :L[p]].tolist() for a in full[:-1]))) for p in range(dev.P)]


def _assert_equals_restated(dev, lists, cur, k, base, wide, what):
    page = dev.topk(k, base, after=cur, wide=wide)
    for p in range(dev.P):
        c = tuple(int(a[p]) for a in cur)
        want = resumed(lists[p], c, k)
        got = list(zip(*(a[p, :page[-1][p]].tolist() for a in page[:-1])))
        assert got == want, (what, p, c)
        assert page[-1][p] == len(want)
        assert (page[-2][p, len(want):] == I32_MAX).all()
        assert (page[0][p, len(want):] == I64_MAX).all()


@pytest.mark.gpu
def test_sentinels_and_arbitrary_cursors(ctx):
    c = paging_case(8, None)
    dev = Dev(ctx, c)
    k = 16
    plain = dev.topk(k, BASE)
    begin = dev.topk(k, BASE, after=(np.full(P, I64_MIN), np.full(P, -1)))
    for a, b in zip(begin, plain):
        assert a.tobytes() == b.tobytes()
    end = dev.topk(k, BASE, after=(np.full(P, I64_MAX), np.full(P, I32_MAX)))
    assert (end[2] == 0).all() and (end[0] == I64_MAX).all() and (end[1] == I32_MAX).all()
    lists = _full_lists(dev, BASE)
    assert sum(len(x) > 100 for x in lists) > P // 2
    rng = np.random.default_rng(0xC0)
    # a record of the middle of each list (the begin cursor for an empty one)
    mid = [x[len(x) // 2] if x else (I64_MIN, -1) for x in lists]
    mk, mn = np.array([m[0] for m in mid]), np.array([m[1] for m in mid])
    absent = np.array([rng.choice(np.setdiff1d(np.arange(BASE, BASE + N), [r[1] for r in x]))
                       for x in lists])
    # (the metric's values are whole multiples of 1 000: key + 1 lies strictly between two)
    variants = {"a node absent from the list": (mk, absent),
                "a node below node_base": (mk, np.full(P, BASE - 5)),
                "a node below node_base, negative": (mk, np.full(P, -7)),
                "a node past the shard": (mk, np.full(P, BASE + N + 7)),
                "a key between two values": (mk + 1, mn),
                "a key between two values, below": (mk - 1, np.full(P, I32_MAX)),
                "random": (rng.integers(-2, 8001, P) * rng.choice([1, -1], P),
                           rng.integers(-10, BASE + N + 10, P))}
    # inside the ranges the walk jumps over: the tie runs of the values 6 and 0 of metric 0 are
    # excluded by the rules of pods 0, 2 and 3 (0 too: 6 lies in its GreaterThan 5 range)
    op = c["prio"]["op"]
    for val in (6000, 0):
        key_of = np.where(op == GT, -val - 1, np.where(op == LT, val, 0))
        variants[f"inside the run of {val}"] = (key_of, np.full(P, BASE + N // 2))
    for what, cur in variants.items():
        _assert_equals_restated(dev, lists, cur, k, BASE, False, what)


# ------------------------------------------------------------------ 3. wide records
@functools.lru_cache(maxsize=None)
def wide_cases():
    """(mixed, narrow3, held_wide).  mixed is test_topk_wide's C5 case: the prioritize columns
    are wide (1, 4: wholes 0..50 with nano 0 and != 0 on every whole, so ties in the nano alone
    and equal pairs on different nodes), narrow at scale 0 (2), at scale 6 (5) and milli (0, 3).
    narrow3 holds columns 1 and 4 as milli values (whole * 1000 + one of 0, 1, 500, 999) and
    every column at scale 3; held_wide holds the same values of columns 1 and 4 wide."""
    from test_topk_wide import c5_case
    rng = np.random.default_rng(0xAF73)
    mixed = c5_case(rng, N, P, 8, 1500)
    narrow3 = dict(mixed)
    v = mixed["v"].copy()
    held = {}
    for m in (1, 4):
        v[m] = mixed["wide"][m][0] * 1000 + rng.choice(np.array([0, 1, 500, 999]), N)
        held[m] = (v[m] // 1000, ((v[m] % 1000) * 10**6).astype(np.uint32))
    v[2], v[5] = mixed["v"][2] * 1000, mixed["v"][5] // 1000  # (the same values at scale 3)
    narrow3.update(v=v, scale=[3] * 6, wide={})
    held_wide = dict(narrow3, wide=held)
    for c in (mixed, narrow3, held_wide):
        c["cand"] = None
    return mixed, narrow3, held_wide


@pytest.mark.gpu
@pytest.mark.parametrize("k", [7, 16])
def test_wide_pages_equal_long_wide_list(ctx, k):
    mixed, narrow3, held_wide = wide_cases()
    # nano-only ties and equal pairs on different nodes in the wide prioritize column
    w, f = mixed["wide"][1]
    pairs = w * 10**9 + f
    assert len(np.unique(pairs)) < N // 4 and len(np.unique(w)) < len(np.unique(pairs))
    for name, c in (("mixed", mixed), ("narrow3", narrow3), ("held_wide", held_wide)):
        dev = Dev(ctx, c, scale=c["scale"], wide=c["wide"])
        full = check_paging(dev, k, BASE, wide=True)
        pm = c["prio"]["metric"][full[-1] > 2 * k]
        if name == "mixed":  # paged pods on the wide, the scale-0 and the scale-6 columns
            assert {2, 5} <= set(pm.tolist()) and {1, 4} & set(pm.tolist())


@pytest.mark.gpu
def test_wide_cursors_are_in_the_canonical_unit(ctx):
    """Cursors taken from the pages of a scale-3 snapshot, applied to the same values held
    wide, return the same records; arbitrary cursors equal the restatement on both."""
    _, narrow3, held_wide = wide_cases()
    k = 16
    dn = Dev(ctx, narrow3, scale=narrow3["scale"], wide=narrow3["wide"])
    pages = [dn.topk(k, BASE, wide=True)]
    for _ in range(3):
        pages.append(dn.topk(k, BASE, after=last_record(pages[-1], k), wide=True))
    lists = _full_lists(dn, BASE, wide=True)
    assert (pages[2][-1] == k).mean() > 1 / 3
    rng = np.random.default_rng(0xC1)
    mid = [x[len(x) // 3] if x else (I64_MIN, 0, -1) for x in lists]
    mk, ms, mn = (np.array([m[j] for m in mid]) for j in range(3))
    variants = {"sub + 1": (mk, np.minimum(ms + 1, U32_MAX), np.full(P, -1)),
                "sub - 1": (mk, np.maximum(ms - 1, 0), np.full(P, I32_MAX)),
                "a node past the shard": (mk, ms, np.full(P, BASE + N + 1)),
                "random": (rng.integers(-60, 60, P), rng.choice([0, 1, 10**9, U32_MAX], P),
                           rng.integers(-10, BASE + N + 10, P))}
    for what, cur in variants.items():
        _assert_equals_restated(dn, lists, cur, k, BASE, True, what)
    # the same values held wide (the context's snapshot is replaced)
    dw = Dev(ctx, held_wide, scale=held_wide["scale"], wide=held_wide["wide"])
    for i in range(3):
        got = dw.topk(k, BASE, after=last_record(pages[i], k), wide=True)
        for a, b in zip(got, pages[i + 1]):
            np.testing.assert_array_equal(a, b, f"page {i + 1}")
    for what, cur in variants.items():
        _assert_equals_restated(dw, lists, cur, k, BASE, True, what + ", held wide")


# ------------------------------------------------------------------ 4. two shards, one GPU
@pytest.mark.gpu
def test_two_shards_resume_after_one_global_cursor(ctx):
    c = paging_case(8, 0.8)
    k = 16
    one = Dev(ctx, c)
    # cursors inside the lists' first tie runs: record 40 of each list (the padding record
    # where the list is shorter), and for the odd pods the same key with a node of the other
    # half of the cluster: not a record, and in the other shard than the even pods' nodes
    deep = one.topk(41, 0)
    ck, cn = deep[0][:, 40].copy(), deep[1][:, 40].copy()
    odd = (np.arange(P) % 2 == 1) & (cn != I32_MAX)
    cn[odd] = (cn[odd] + N // 2) % N
    cur = (ck, cn)
    want = one.topk(k, 0, after=cur)
    assert (want[2] == k).mean() > 1 / 3
    halves = [node_range(N, 2, r) for r in range(2)]
    # the cursor's node lies in either shard, for a good share of the pods each
    real = cur[1] != I32_MAX
    for n0, n1 in halves:
        assert ((cur[1] >= n0) & (cur[1] < n1) & real).mean() >= 0.25
    recs = []
    for n0, n1 in halves:
        with pas_amd.Context(0) as c2:
            recs.append(Dev(c2, c, n0, n1).topk(k, n0, after=cur))
    keys_all = _dev(np.stack([r[0] for r in recs]))
    nodes_all = _dev(np.stack([r[1] for r in recs]))
    out_node = torch.empty((P, k), dtype=torch.int32, device="cuda")
    out_len = torch.empty(P, dtype=torch.int32, device="cuda")
    ctx.topk_merge_device(P, k, 2, keys_all, nodes_all, out_node, out_len)
    ctx.synchronize()
    np.testing.assert_array_equal(out_len.cpu().numpy(), want[2])
    np.testing.assert_array_equal(out_node.cpu().numpy(),
                                  np.where(want[1] == I32_MAX, -1, want[1]))


# ------------------------------------------------------------------ 5. errors
@pytest.mark.gpu
def test_after_errors(ctx):
    mixed, narrow3, _ = wide_cases()
    k = 4
    dev = Dev(ctx, narrow3, scale=narrow3["scale"], wide={})
    head = (dev.tas_gen, dev.gas_gen, P, dev.nr, *dev.tas, *dev.gas, k, 0)
    key = torch.full((P, k), -3, dtype=torch.int64, device="cuda")
    sub = torch.full((P, k), -3, dtype=torch.int32, device="cuda")
    node = torch.full((P, k), -3, dtype=torch.int32, device="cuda")
    ln = torch.full((P,), -3, dtype=torch.int32, device="cuda")
    ak, an = _dev(np.full(P, I64_MIN)), _dev(np.full(P, -1, np.int32))
    asub = _dev(np.zeros(P, np.int32))
    for cur in ((None, an), (ak, None)):
        with pytest.raises(pas_amd.PasError) as e:
            ctx.tas_gas_topk_after_device(*head, *cur, key, node, ln)
        assert e.value.code == _lib.PAS_EINVAL
    for cur in ((None, asub, an), (ak, None, an), (ak, asub, None)):
        with pytest.raises(pas_amd.PasError) as e:
            ctx.tas_gas_topk_wide_after_device(*head, *cur, key, sub, node, ln)
        assert e.value.code == _lib.PAS_EINVAL
    # no pods: nothing is read or written, null arrays included
    none = (dev.tas_gen, dev.gas_gen, 0, dev.nr, *dev.tas, *dev.gas, k, 0)
    ctx.tas_gas_topk_after_device(*none, None, None, key, node, ln)
    ctx.tas_gas_topk_wide_after_device(*none, None, None, None, key, sub, node, ln)
    ctx.synchronize()
    assert (key == -3).all() and (node == -3).all() and (ln == -3).all() and (sub == -3).all()
    # the 64-bit records on a snapshot with wide columns
    dev = Dev(ctx, mixed, scale=mixed["scale"], wide=mixed["wide"])
    head = (dev.tas_gen, dev.gas_gen, P, dev.nr, *dev.tas, *dev.gas, k, 0)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_gas_topk_after_device(*head, ak, an, key, node, ln)
    assert e.value.code == _lib.PAS_ENOTEXACT
    ctx.tas_gas_topk_wide_after_device(*head, ak, asub, an, key, sub, node, ln)
    ctx.synchronize()
