"""Top-k over wide metric columns: the wide merge records (key, sub, node) of include/pas.h
("Wide merge records"), their two producers (pas_tas_topk_wide_device,
pas_tas_gas_topk_wide_device), their two merges (pas_topk_merge_wide_device,
pas_list_merge_wide_device) and the `wide=` argument of pas_amd/shard.py.

Checkers: the oracle's per-value decimal form (oracle.tas_eval(..., v_scale=s)) wherever the
values are oracle-representable, `Restated` (test_wide_columns.py) for the mixed-form cluster.
The expected records come from `canon` / `record` below, a restatement of the record contract
on Python ints / NumPy, which the CPU tests first show equal to the exact Decimal order.
"""
import decimal
import os
import sys
from decimal import Decimal

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import pas_amd
from pas_amd.workload import pack_bits
from helpers import RULE_DTYPE, unpack_bits
from test_quantity_scaled import go_value
from test_wide_columns import (COUNTER, MIXED, PAST, Restated, random_wide, rule_batch,
                               wide_oracle_values, wide_pair)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT, GT, EQ = 0, 1, 2
I64_MAX, I64_MIN = 2**63 - 1, -2**63
U32_MAX, I32_MAX = 2**32 - 1, 2**31 - 1
ECAPACITY = pas_amd._lib.PAS_ECAPACITY


# ------------------------------------------------------------------ the restatement (pas.h)
def canon(v: int, s: int):
    """The canonical pair (W, F) of the narrow value v held at multiplier 10^s."""
    W = v // 10**s  # Python's // floors toward -inf
    return W, (v - W * 10**s) * 10**(9 - s)


def record(op: int, W: int, F: int):
    """(key, sub) of the pair under the prioritize operator: key as int64, sub as uint32."""
    if op == LT:
        return W, F
    if op == GT:
        return -W - 1, U32_MAX - F  # ~W, ~F
    return 0, 0


def canon_cols(v, scale, wide):
    """W int64 [M][N], F uint32 [M][N] of a snapshot: narrow columns v at `scale`, wide columns
    {m: (whole, nano)}."""
    W = np.zeros(v.shape, np.int64)
    F = np.zeros(v.shape, np.uint32)
    for m in range(v.shape[0]):
        if m in wide:
            W[m], F[m] = wide[m]
        else:
            mult = np.int64(10**int(scale[m]))
            W[m] = np.floor_divide(v[m], mult)
            F[m] = ((v[m] - W[m] * mult) * np.int64(10**(9 - int(scale[m])))).astype(np.uint32)
    return W, F


def expected_records(order, lens, prio, W, F, k, base):
    """Records of the first k entries of the checker's lists (order [P][N], lens [P])."""
    P = len(prio)
    keys = np.full((P, k), I64_MAX, np.int64)
    subs = np.full((P, k), U32_MAX, np.uint32)
    nodes = np.full((P, k), I32_MAX, np.int32)
    ln = np.minimum(lens, k).astype(np.int32)
    for p in range(P):
        n = int(ln[p])
        if n == 0:
            continue
        loc, m, op = order[p, :n], int(prio["metric"][p]), int(prio["op"][p])
        nodes[p, :n] = loc + base
        if op == LT:
            keys[p, :n], subs[p, :n] = W[m, loc], F[m, loc]
        elif op == GT:
            keys[p, :n], subs[p, :n] = np.invert(W[m, loc]), np.invert(F[m, loc])
        else:
            keys[p, :n], subs[p, :n] = 0, 0
    return keys, subs, nodes, ln


# ------------------------------------------------------------------ CPU tests
def _order_by_records(pairs, op):
    recs = [record(op, W, F) + (n,) for n, (W, F) in enumerate(pairs)]
    return [n for _, _, n in sorted(recs)]


def test_record_order_is_the_exact_value_order():
    """Ascending (key, sub, node) of the restated records = Restated's HostPriorityList order,
    on the wide literals and on 2 000 random pairs, for both operators."""
    rng = np.random.default_rng(0x70B)
    with decimal.localcontext() as c:
        c.prec = 80
        cols = [[go_value(lit) for lit in col] for col in (COUNTER, MIXED, PAST)]
        whole, nano = random_wide(rng, 2000)
        # and pairs past the oracle's form: any whole with any nano
        far = rng.random(2000) < 0.3
        nano[far] = rng.integers(0, 10**9, int(far.sum()))
        cols.append([Decimal(int(w)) + Decimal(int(f)).scaleb(-9) for w, f in zip(whole, nano)])
        for vals in cols:
            pairs = [wide_pair(v) for v in vals]
            rs = Restated([vals])
            for op in (LT, GT):
                prio = np.array([(0, op, 0)], RULE_DTYPE)
                _, order, lens = rs.tas_eval(np.zeros(0, RULE_DTYPE), np.zeros(2, np.int32), prio)
                assert lens[0] == len(vals)
                assert _order_by_records(pairs, op) == list(order[0, :lens[0]]), op
                for W, F in pairs:
                    key, sub = record(op, W, F)
                    assert I64_MIN <= key <= I64_MAX and 0 <= sub <= U32_MAX


def test_narrow_value_to_canonical_pair():
    """canon(v, s) = wide_pair(v * 10^-s) over the whole int64 range, s = 0..9, and the NumPy
    form used for the expected records agrees with it."""
    rng = np.random.default_rng(0x70C)
    with decimal.localcontext() as c:
        c.prec = 80
        edge = [I64_MIN, I64_MIN + 1, -1500, -1000, -999, -1, 0, 1, 999, 1000, 1500, I64_MAX - 1,
                I64_MAX]
        vs = edge + [int(x) for x in rng.integers(I64_MIN, I64_MAX, 3000, dtype=np.int64,
                                                  endpoint=True)]
        vs += [int(x) for x in rng.integers(-10**10, 10**10, 1000)]
        for s in range(10):
            for v in vs:
                W, F = canon(v, s)
                assert (W, F) == wide_pair(Decimal(v).scaleb(-s)), (v, s)
                assert 0 <= F < 10**9
            arr = np.array(vs, np.int64)[None, :]
            Wn, Fn = canon_cols(arr, [s], {})
            assert [(int(a), int(b)) for a, b in zip(Wn[0], Fn[0])] == [canon(v, s) for v in vs]
    assert canon(-1500, 3) == (-2, 500000000)


# ------------------------------------------------------------------ GPU helpers
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rule_tensors(rules, off, prio, cand):
    return (_dev(rules.view(np.uint8)), _dev(off), _dev(prio.view(np.uint8)),
            None if cand is None else _dev(cand.view(np.int64)))


def _bufs(P, k):
    return (torch.empty((P, k), dtype=torch.int64, device="cuda"),
            torch.empty((P, k), dtype=torch.int32, device="cuda"),
            torch.empty((P, k), dtype=torch.int32, device="cuda"),
            torch.empty(P, dtype=torch.int32, device="cuda"))


def _host(key, sub, node, ln):
    return (key.cpu().numpy(), sub.cpu().numpy().view(np.uint32), node.cpu().numpy(),
            ln.cpu().numpy())


def topk_wide(ctx, gen, rules, off, prio, cand, k, base):
    P = len(prio)
    key, sub, node, ln = _bufs(P, k)
    ctx.tas_topk_wide_device(gen, P, len(rules), *_rule_tensors(rules, off, prio, cand), k, base,
                             key, sub, node, ln)
    ctx.synchronize()
    return _host(key, sub, node, ln)


def assert_records(got, want, what=""):
    for g, w, name in zip(got, want, ("key", "sub", "node", "len")):
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")


def set_snapshot(ctx, gen, v, pres, scale, wide):
    """Narrow columns at `scale`, then the wide columns {m: (whole, nano)}; returns the
    generation to evaluate against."""
    ctx.tas_snapshot_set(gen, v, pres, scale=np.asarray(scale, np.int32))
    if not wide:
        return gen
    cols = sorted(wide)
    ctx.tas_snapshot_update_wide(gen, gen + 1, cols, np.stack([wide[m][0] for m in cols]),
                                 np.stack([wide[m][1] for m in cols]), pres[cols])
    return gen + 1


def oracle_form(v, scale, wide):
    """(u, s) per value for the oracle: narrow columns at their scale, wide columns through
    wide_oracle_values."""
    u = v.copy()
    s = np.repeat(np.asarray(scale, np.int8)[:, None], v.shape[1], 1)
    for m, (whole, nano) in wide.items():
        u[m], s[m] = wide_oracle_values(whole, nano)
    return u, s


# ------------------------------------------------------------------ 1. records
_RECORDS = {}


def records_case(oracle):
    """N = 4 097 (past a bitmap word and the 1 024-position segments), two wide columns, one
    narrow at scale 4, one narrow milli; 64 pods.  The checker's lists are computed once."""
    if _RECORDS:
        return _RECORDS
    rng = np.random.default_rng(0x4097)
    N, M, P = 4097, 4, 64
    scale = [3, 3, 4, 3]
    v = np.zeros((M, N), np.int64)
    v[2] = rng.choice(rng.integers(-60000, 60000, 300), N)  # scale 4, heavy ties
    v[3] = rng.choice(rng.integers(-6000, 6000, 300), N)    # milli
    wide = {0: random_wide(rng, N), 1: random_wide(rng, N)}
    pres = pack_bits(rng.random((M, N)) < 0.93)
    # targets on existing wholes (the small class has nano = 0 and != 0 on the same whole)
    targets = list(range(-6, 7)) + [I64_MAX, I64_MIN, -I64_MAX, 10**9, -10**9] + \
        [int(w) for w in wide[0][0][:6]]
    rules, off, prio = rule_batch(rng, M, P, 2, targets)
    prio["op"][:8] = [LT, GT, EQ, LT, GT, EQ, LT, GT]
    prio["metric"][:8] = [0, 0, 0, 1, 1, 2, 2, 3]
    prio["metric"][8] = 99   # not cached: empty list
    prio["metric"][9] = M
    off[1:5] = off[0]        # pods 0..3: no rules (the whole order), the rest keep theirs
    cand = pack_bits(rng.random((P, N)) < 0.9)
    u, s = oracle_form(v, scale, wide)
    _, order, lens = oracle.tas_eval(u, pres, rules, off, prio, cand, v_scale=s)
    W, F = canon_cols(v, scale, wide)
    assert lens[8] == 0 and lens[9] == 0 and lens[0] > 3000 and (lens > 300).sum() >= 4
    _RECORDS.update(v=v, pres=pres, scale=scale, wide=wide, rules=rules, off=off, prio=prio,
                    cand=cand, order=order, lens=lens, W=W, F=F)
    return _RECORDS


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 16, 300])
def test_wide_records_match_checker(ctx, oracle, k):
    c = records_case(oracle)
    gen = set_snapshot(ctx, 7100, c["v"], c["pres"], c["scale"], c["wide"])
    assert ctx.tas_snapshot_wide_count() == 2
    base = 1234
    got = topk_wide(ctx, gen, c["rules"], c["off"], c["prio"], c["cand"], k, base)
    want = expected_records(c["order"], c["lens"], c["prio"], c["W"], c["F"], k, base)
    assert_records(got, want, f"k={k}")


# ------------------------------------------------------------------ 2. narrow snapshot
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 16, 300])
def test_wide_records_on_a_narrow_snapshot(ctx, k):
    """No wide column (nano / wide_flag are null): nodes and lengths are
    pas_tas_topk_device's, key / sub the canonical form of its keys."""
    from test_shard import make_case
    snap, batch = make_case(0x7A, 4100, 6, 48, 5, cand_frac=0.9)
    v, pres = snap.v_milli, snap.present
    scale = [3, 0, 9, 3, 6, 3]
    gen = set_snapshot(ctx, 7200, v, pres, scale, {})
    assert ctx.tas_snapshot_wide_count() == 0
    P = len(batch.prio)
    tensors = _rule_tensors(batch.rules, batch.rule_off, batch.prio, batch.cand)
    key, _, node, ln = _bufs(P, k)
    ctx.tas_topk_device(gen, P, len(batch.rules), *tensors, k, 77, key, node, ln)
    ctx.synchronize()
    nkey, nnode, nlen = key.cpu().numpy(), node.cpu().numpy(), ln.cpu().numpy()
    gkey, gsub, gnode, glen = topk_wide(ctx, gen, batch.rules, batch.rule_off, batch.prio,
                                        batch.cand, k, 77)
    np.testing.assert_array_equal(gnode, nnode)
    np.testing.assert_array_equal(glen, nlen)
    assert (nlen > 0).sum() > 10
    for p in range(P):
        op, m = int(batch.prio["op"][p]), int(batch.prio["metric"][p])
        for j in range(k):
            if j >= nlen[p]:
                assert (gkey[p, j], gsub[p, j], gnode[p, j]) == (I64_MAX, U32_MAX, I32_MAX)
                continue
            val = int(nkey[p, j]) if op == LT else -int(nkey[p, j]) - 1 if op == GT else 0
            want = record(op, *canon(val, scale[m])) if op in (LT, GT) else (0, 0)
            assert (int(gkey[p, j]), int(gsub[p, j])) == want, (p, j)


# ------------------------------------------------------------------ 3. mixed forms
def mixed_cluster(seed, N):
    """One metric (0) held narrow at scale 3 on shard 0, narrow at scale 6 on shard 1 and
    wide on the rest; values are multiples of 0.001 from a small pool (representable in every
    form, equal across shards).  Metrics 1, 2: milli on every shard."""
    rng = np.random.default_rng(seed)
    M, P = 3, 24
    v = np.zeros((M, N), np.int64)  # the cluster in milli
    v[0] = rng.choice(rng.integers(-4000, 4000, 40), N)
    v[1:] = rng.choice(rng.integers(-4000, 4000, 200), (2, N))
    pres_b = rng.random((M, N)) < 0.93
    rules, off, prio = rule_batch(rng, M, P, 2, [-4, -3, -1, 0, 1, 2, 3, 4])
    prio["metric"][:16] = 0
    prio["op"][:16] = [LT, GT] * 8
    prio["op"][16] = EQ
    off[1:4] = off[0]
    cand = pack_bits(rng.random((P, N)) < 0.9)
    with decimal.localcontext() as c:
        c.prec = 80
        vals = [[Decimal(int(x)).scaleb(-3) if pres_b[m, n] else None
                 for n, x in enumerate(v[m])] for m in range(M)]
        _, order, lens = Restated(vals).tas_eval(rules, off, prio, cand)
    return v, pres_b, rules, off, prio, cand, order, lens


def shard_form(v, pres_b, n0, n1, r):
    sv = np.ascontiguousarray(v[:, n0:n1])
    sp = pack_bits(pres_b[:, n0:n1])
    if r == 0:
        return sv, sp, [3, 3, 3], {}
    if r == 1:
        sv[0] *= 1000
        return sv, sp, [6, 3, 3], {}
    whole = np.floor_divide(sv[0], 1000)
    nano = ((sv[0] - whole * 1000) * 10**6).astype(np.uint32)
    sv[0] = 0
    return sv, sp, [3, 3, 3], {0: (whole, nano)}


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3, 8])
def test_mixed_forms_across_shards(ctx, world):
    from pas_amd.shard import node_range
    N = 1500
    v, pres_b, rules, off, prio, cand, order, lens = mixed_cluster(0x3F + world, N)
    P = len(prio)
    width = node_range(N, world, 0)[1]
    ks = [1, 7, 16, width]
    recs = {k: [] for k in ks}
    for r in range(world):
        n0, n1 = node_range(N, world, r)
        sv, sp, scale, wide = shard_form(v, pres_b, n0, n1, r)
        gen = set_snapshot(ctx, 7300 + 2 * r, sv, sp, scale, wide)
        scand = pack_bits(unpack_bits(cand, N)[:, n0:n1])
        t = _rule_tensors(rules, off, prio, scand)
        for k in ks:
            key, sub, node, ln = _bufs(P, k)
            ctx.tas_topk_wide_device(gen, P, len(rules), *t, k, n0, key, sub, node, ln)
            recs[k].append((key, sub, node))
        ctx.synchronize()
    # equal values in different forms give equal (key, sub): the tie is broken by node alone
    k0 = recs[width][0][0].cpu().numpy()
    k1 = recs[width][1][0].cpu().numpy()
    assert np.intersect1d(k0[0][k0[0] != I64_MAX], k1[0][k1[0] != I64_MAX]).size > 0
    out_len = torch.empty(P, dtype=torch.int32, device="cuda")
    for k in ks:
        keys, subs, nodes = (torch.stack([x[i] for x in recs[k]]) for i in range(3))
        if k == width:
            out = torch.empty((P, world * width), dtype=torch.int32, device="cuda")
            ctx.list_merge_wide_device(P, world, width, keys, subs, nodes, out, out_len)
        else:
            out = torch.empty((P, k), dtype=torch.int32, device="cuda")
            ctx.topk_merge_wide_device(P, k, world, keys, subs, nodes, out, out_len)
        ctx.synchronize()
        got, gl = out.cpu().numpy(), out_len.cpu().numpy()
        for p in range(P):
            n = min(int(lens[p]), k) if k != width else int(lens[p])
            assert gl[p] == n, (k, p)
            np.testing.assert_array_equal(got[p, :n], order[p, :n], err_msg=f"k={k} pod {p}")
            assert (got[p, n:] == -1).all()


# ------------------------------------------------------------------ 4. merge kernels alone
def synthetic_runs(rng, S, P, w):
    """Sorted runs [S][P][w] of records that mostly differ only in sub or only in node, with
    all-sentinel runs; node ids distinct per pod."""
    keys = np.full((S, P, w), I64_MAX, np.int64)
    subs = np.full((S, P, w), U32_MAX, np.uint32)
    nodes = np.full((S, P, w), I32_MAX, np.int32)
    for p in range(P):
        ids = rng.permutation(S * w).astype(np.int32)
        for s in range(S):
            n = 0 if (s + p) % 4 == 3 else int(rng.integers(0, w + 1)) if p else w
            k = rng.choice(np.array([0, 1, -1, I64_MAX], np.int64), n)
            f = rng.choice(np.array([0, 1, U32_MAX - 1, U32_MAX], np.uint32), n)
            if p == 1:
                k[:] = 5  # only sub and node differ
            if p == 2:
                k[:], f[:] = 5, 9  # only node differs
            nd = ids[s * w:s * w + n]
            o = np.lexsort((nd, f, k))
            keys[s, p, :n], subs[s, p, :n], nodes[s, p, :n] = k[o], f[o], nd[o]
    return keys, subs, nodes


def merged(keys, subs, nodes, p):
    k, f, nd = keys[:, p].ravel(), subs[:, p].ravel(), nodes[:, p].ravel()
    real = nd != I32_MAX
    k, f, nd = k[real], f[real], nd[real]
    return nd[np.lexsort((nd, f, k))]


@pytest.mark.gpu
@pytest.mark.parametrize("S,k", [(1, 1), (4, 16), (8, 512)])
def test_topk_merge_wide_kernel(ctx, S, k):
    rng = np.random.default_rng(0x44 + S)
    P = 6
    keys, subs, nodes = synthetic_runs(rng, S, P, k)
    out = torch.empty((P, k), dtype=torch.int32, device="cuda")
    out_len = torch.empty(P, dtype=torch.int32, device="cuda")
    ctx.topk_merge_wide_device(P, k, S, _dev(keys), _dev(subs.view(np.int32)), _dev(nodes), out,
                               out_len)
    ctx.synchronize()
    got, gl = out.cpu().numpy(), out_len.cpu().numpy()
    for p in range(P):
        want = merged(keys, subs, nodes, p)[:k]
        assert gl[p] == len(want)
        np.testing.assert_array_equal(got[p, :len(want)], want, err_msg=f"pod {p}")
        assert (got[p, len(want):] == -1).all()


@pytest.mark.gpu
def test_topk_merge_wide_capacity(ctx):
    """16 bytes of LDS per wide record: n_shards * k = 4 096 runs (above), 4 097 does not."""
    k = 4097
    z = torch.zeros((1, k), dtype=torch.int64, device="cuda")
    z32 = torch.zeros((1, k), dtype=torch.int32, device="cuda")
    with pytest.raises(pas_amd.PasError) as e:
        ctx.topk_merge_wide_device(1, k, 1, z, z32, z32, z32.clone(),
                                   torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert e.value.code == ECAPACITY


@pytest.mark.gpu
@pytest.mark.parametrize("S,w", [(1, 5), (2, 1), (3, 700), (8, 1024)])
def test_list_merge_wide_kernel(ctx, S, w):
    rng = np.random.default_rng(0x55 + S * w)
    P = 4
    keys, subs, nodes = synthetic_runs(rng, S, P, w)
    out = torch.full((P, S * w + 3), -7, dtype=torch.int32, device="cuda")
    out_len = torch.empty(P, dtype=torch.int32, device="cuda")
    ctx.list_merge_wide_device(P, S, w, _dev(keys), _dev(subs.view(np.int32)), _dev(nodes), out,
                               out_len, out_ld=S * w + 3)
    ctx.synchronize()
    got, gl = out.cpu().numpy(), out_len.cpu().numpy()
    for p in range(P):
        want = merged(keys, subs, nodes, p)
        assert gl[p] == len(want)
        np.testing.assert_array_equal(got[p, :len(want)], want, err_msg=f"pod {p}")
        assert (got[p, len(want):S * w] == -1).all() and (got[p, S * w:] == -7).all()


# ------------------------------------------------------------------ 5. C5 wide
def c5_case(rng, n, P, cards, jump, long_pod=True):
    """TAS: 6 metrics, columns 1 and 4 wide (wholes 0..50 with heavy ties, nano 0 and != 0 on
    every whole), the rest narrow at mixed scales.  Pods 0..5 prioritize wide column 1 under a
    rule on the same column whose target T sits on such a tie: GreaterThan / GreaterThan and
    LessThan / LessThan exclude the first `jump` positions of their own order, Equals rules
    under both orders; pod 6 (long_pod) has 40 rules, so its wave takes the unstaged path."""
    from pas_amd import workload as wl
    from test_gas_gpu import random_gas
    M = 6
    scale = [3, 3, 0, 3, 3, 6]
    v = np.zeros((M, n), np.int64)
    for m in (0, 3):
        v[m] = rng.choice(rng.integers(-5000, 60000, 200), n)
    v[2] = rng.integers(-3, 55, n)
    v[5] = rng.choice(rng.integers(-5, 55, 100) * 10**6 + rng.integers(0, 3, 100) * 500000, n)
    wide = {}
    for m in (1, 4):
        whole = rng.integers(0, 51, n).astype(np.int64)
        nano = rng.choice(np.array([0, 0, 1, 500_000_000, 999_999_999], np.uint32), n)
        wide[m] = (whole, nano)
    pres = pack_bits(rng.random((M, n)) < 0.95)
    targets = [-1, 0, 1, 3, 25, 48, 49, 50, 51, 60]
    rules, off, prio = rule_batch(rng, M, P, 3, targets)
    # a rule hits ~half the nodes: keep the first of each pod's three, neutralise some others
    rules["metric"][rng.random(len(rules)) < 0.5] = 99  # not cached: the rule is skipped
    w1 = np.sort(wide[1][0])
    t_gt = int(w1[min(max(n - jump, 0), n - 1)])  # ~jump nodes have whole >= t_gt
    t_lt = int(w1[min(jump, n - 1)])       # ~jump nodes have whole <= t_lt
    special = [((1, GT), [(1, GT, t_gt)]), ((1, LT), [(1, LT, t_lt)]),
               ((1, GT), [(1, EQ, int(w1[-1]))]), ((1, LT), [(1, EQ, int(w1[0]))]),
               ((1, GT), [(1, GT, t_gt), (4, EQ, 25)]), ((4, LT), [(4, GT, 25), (1, LT, 3)])]
    if long_pod:
        miss = [(LT, -10), (GT, 70), (EQ, 61)]  # no value is below -10, above 70 or 61
        special.append(((4, GT), [(int(rng.integers(0, M)),) + miss[int(rng.integers(0, 3))]
                                  for _ in range(38)] + [(4, EQ, 50), (1, GT, 49)]))
    per_pod = [list(map(tuple, rules[off[p]:off[p + 1]])) for p in range(P)]
    for p, (pr, rl) in enumerate(special):
        per_pod[p] = rl
        prio[p] = pr + (0,)
    prio["metric"][P - 1] = 99  # no scheduling rule: empty list
    rules = np.array([r for rl in per_pod for r in rl], RULE_DTYPE)
    off = np.cumsum([0] + [len(rl) for rl in per_pod]).astype(np.int32)
    if cards == 8:
        seed = int(rng.integers(1, 1 << 30))
        gs, gb = wl.make_gas_snapshot(n, seed=seed), wl.make_gas_batch(P, seed=seed)
        i915 = wl.I915
    else:
        nc, cap, used, req, mask, ncont = random_gas(rng, n, cards, 3, P, 4, i915=0)
        cap *= 4
        gs, gb, i915 = wl.GasSnapshotData(nc, cap, used), wl.GasBatch(req, mask, ncont), 0
    return dict(v=v, pres=pres, scale=scale, wide=wide, rules=rules, off=off, prio=prio, gs=gs,
                gb=gb, i915=i915)


def c5_expected(oracle, c, cand, k, base):
    n = c["v"].shape[1]
    gs, gb = c["gs"], c["gb"]
    fit = (oracle.gas_fit(gs.n_cards, gs.cap, gs.used, gb.req, gb.req_mask, gb.n_containers,
                          c["i915"]) >> 31).astype(bool)
    if cand is not None:
        fit &= unpack_bits(cand, n)
    u, s = oracle_form(c["v"], c["scale"], c["wide"])
    _, order, lens = oracle.tas_eval(u, c["pres"], c["rules"], c["off"], c["prio"],
                                     pack_bits(fit), v_scale=s)
    W, F = canon_cols(c["v"], c["scale"], c["wide"])
    return expected_records(order, lens, c["prio"], W, F, k, base)


def c5_run(ctx, c, cand, k, base, gen, composed=True):
    """(lazy records, composed records): pas_tas_gas_topk_wide_device, and
    pas_gas_fit_bitmap_device -> pas_tas_topk_wide_device with the fit bitmaps as candidates."""
    n = c["v"].shape[1]
    P = len(c["prio"])
    gs, gb = c["gs"], c["gb"]
    gen_t = set_snapshot(ctx, gen, c["v"], c["pres"], c["scale"], c["wide"])
    ctx.gas_snapshot_set(gen + 5, gs.n_cards, gs.cap, gs.used)
    rules_t, off_t, prio_t, cand_t = _rule_tensors(c["rules"], c["off"], c["prio"], cand)
    req_t, mask_t = _dev(gb.req), _dev(gb.req_mask.view(np.int32))
    nc_t = _dev(gb.n_containers)
    C = gb.req.shape[1]
    key, sub, node, ln = _bufs(P, k)
    ctx.tas_gas_topk_wide_device(gen_t, gen + 5, P, len(c["rules"]), rules_t, off_t, prio_t,
                                 cand_t, C, c["i915"], req_t, mask_t, nc_t, k, base, key, sub,
                                 node, ln)
    ctx.synchronize()
    lazy = _host(key, sub, node, ln)
    if not composed:
        return lazy, None
    fit_t = torch.empty((P, (n + 63) // 64), dtype=torch.int64, device="cuda")
    ctx.gas_fit_bitmap_device(gen + 5, P, C, c["i915"], req_t, mask_t, nc_t, fit_t)
    ctx.synchronize()
    if cand_t is not None:
        fit_t &= cand_t
        torch.cuda.synchronize()
    key, sub, node, ln = _bufs(P, k)
    ctx.tas_topk_wide_device(gen_t, P, len(c["rules"]), rules_t, off_t, prio_t, fit_t, k, base,
                             key, sub, node, ln)
    ctx.synchronize()
    return lazy, _host(key, sub, node, ln)


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,cards,cand_frac,long_pod", [
    (16, 5000, 8, None, True), (1, 3000, 8, 0.7, False), (16, 3000, 12, 0.8, True),
    (16, 5000, 8, 0.9, False), (1, 5000, 12, None, False)])
def test_tas_gas_topk_wide_equals_composition(ctx, oracle, k, n, cards, cand_frac, long_pod):
    """(The jump pods exclude their first ~3 000 positions at n = 5 000, ~2 500 at n = 3 000,
    where 3 000 would leave no node.)"""
    rng = np.random.default_rng(0xC5 + k + n + cards)
    P = 96
    c = c5_case(rng, n, P, cards, min(3000, n - 500), long_pod)
    flag = rng.random(c["gb"].req_mask.shape) < 0.05
    c["gb"].req_mask = c["gb"].req_mask | np.where(flag, 0x80000000, 0).astype(np.uint32)
    cand = None if cand_frac is None else pack_bits(rng.random((P, n)) < cand_frac)
    lazy, composed = c5_run(ctx, c, cand, k, 1234, 7500)
    assert_records(lazy, composed, "lazy vs composed")
    assert_records(lazy, c5_expected(oracle, c, cand, k, 1234), "lazy vs checker")
    # the jump pods list nodes (the jump skipped none that pass) and some pods are empty
    assert (lazy[3] > 0).mean() > 0.2 and lazy[3][P - 1] == 0


# ------------------------------------------------------------------ 6. seeded sweep
@pytest.mark.gpu
def test_wide_record_producers_sweep(ctx, oracle):
    """40 small random shapes, both producers against the checker."""
    for seed in range(40):
        rng = np.random.default_rng(0x5EED + seed)
        n = int(rng.choice([1, 31, 64, 65, 200, 700, 1025]))
        P = int(rng.choice([1, 7, 9, 20]))
        k = int(rng.choice([1, 5, 16, 70]))
        base = int(rng.choice([0, 1234, 1 << 20]))
        c = c5_case(rng, n, max(P, 8), 8, n // 2, long_pod=bool(seed % 3 == 0))
        cand = pack_bits(rng.random((len(c["prio"]), n)) < 0.8) if seed % 2 else None
        if seed % 5 == 0:
            c["wide"] = {}  # a narrow snapshot through the same entry points
            c["v"][[1, 4]] = rng.integers(-3000, 55000, (2, n))
        lazy, composed = c5_run(ctx, c, cand, k, base, 7600 + 10 * seed)
        want = c5_expected(oracle, c, cand, k, base)
        assert_records(lazy, want, f"seed {seed} lazy")
        assert_records(composed, want, f"seed {seed} composed")


# ------------------------------------------------------------------ 7. ShardedTopK(wide=True)
def sharded_case():
    rng = np.random.default_rng(0x5A)
    c = c5_case(rng, 6000, 50, 8, 3000, long_pod=False)
    cand = pack_bits(rng.random((50, 6000)) < 0.85)
    return c, cand


def _gpu_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world),
                      RANK=str(rank), LOCAL_RANK="0")
    for p in (os.path.join(ROOT, "platform-aware-scheduling_amd"), os.path.join(ROOT, "oracle"),
              os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import pas_amd
    from pas_amd import distrib
    from pas_amd.shard import ShardedTopK, node_range

    distrib.setup("gloo")  # ranks share the one GPU: collectives through host memory
    torch.cuda.set_device(0)
    c, cand = sharded_case()
    N = c["v"].shape[1]
    n0, n1 = node_range(N, world, rank)
    sv = np.ascontiguousarray(c["v"][:, n0:n1])
    sp = pack_bits(unpack_bits(c["pres"], N)[:, n0:n1])
    # only rank 1 holds wide columns; rank 0 holds the same metrics narrow at scale 9 (their
    # values fit), so the record form cannot follow the rank's own snapshot
    wide = {m: (w[n0:n1], f[n0:n1]) for m, (w, f) in c["wide"].items()}
    scale = list(c["scale"])
    if rank == 0:
        for m, (w, f) in wide.items():
            sv[m] = w * 10**9 + f.astype(np.int64)
            scale[m] = 9
        wide = {}
    with pas_amd.Context(0) as ctx:
        gen = set_snapshot(ctx, 40, sv, sp, scale, wide)
        assert ctx.tas_snapshot_wide_count() == (0 if rank == 0 else 2)
        t = _rule_tensors(c["rules"], c["off"], c["prio"],
                          pack_bits(unpack_bits(cand, N)[:, n0:n1]))
        st = ShardedTopK(ctx, 12, world, rank, n0, wide=True)
        s = torch.cuda.Stream() if rank == 0 else None
        out_node, out_len = st.run(gen, len(c["prio"]), len(c["rules"]), *t, stream=s)
        torch.cuda.synchronize()
        np.save(os.path.join(out_dir, f"nodes{rank}.npy"), out_node.cpu().numpy())
        np.save(os.path.join(out_dir, f"lens{rank}.npy"), out_len.cpu().numpy())
    distrib.teardown(world)


@pytest.mark.gpu
def test_sharded_topk_wide_two_ranks_one_gpu(tmp_path, oracle):
    """ShardedTopK(wide=True) end to end in two processes (gloo between them, one GPU): rank 0
    holds the two metrics narrow at scale 9, rank 1 wide; both lists equal the checker's."""
    from test_shard import _free_port
    world = 2
    mp.spawn(_gpu_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    c, cand = sharded_case()
    u, s = oracle_form(c["v"], c["scale"], c["wide"])
    _, order, lens = oracle.tas_eval(u, c["pres"], c["rules"], c["off"], c["prio"], cand,
                                     v_scale=s)
    assert (lens > 12).sum() > 5
    for r in range(world):
        nodes = np.load(tmp_path / f"nodes{r}.npy")
        ln = np.load(tmp_path / f"lens{r}.npy")
        for p in range(len(c["prio"])):
            m = min(12, int(lens[p]))
            assert ln[p] == m
            np.testing.assert_array_equal(nodes[p, :m], order[p, :m])
