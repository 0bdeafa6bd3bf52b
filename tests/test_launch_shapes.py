"""The launch paths that depend on the batch or cluster shape, each at the smallest shape that
reaches it: the two pod groupings of the TAS prep and its metric-count branches, the global-pass
eval in several launches, the combined TAS+GAS top-k on nodes past 16 cards, and the node-major
copies of that top-k across a reshape.  Every comparison is bit-exact against the CPU oracle.

The thresholds these shapes rest on are pinned by tests/test_launch_constants.py: if one moves,
the shapes here must move with it.  Marked gpu."""
import functools

import numpy as np
import pytest
import torch

import pas_amd
from pas_amd import _lib
from pas_amd import workload as wl
from helpers import RULE_DTYPE, pack_bits, unpack_bits
from test_gas_wide import random_wide
from test_shard import _dev, _rule_tensors, order_keys
from test_tas_gpu import assert_same, random_case, upload
from test_topk_after import Dev, last_record
from test_topk_wide import c5_expected

pytestmark = pytest.mark.gpu

LT, GT, EQ = 0, 1, 2
I64_MIN, I64_MAX, I32_MAX = -2**63, 2**63 - 1, 2**31 - 1
ORDER_OF = {LT: 0, GT: 1}  # kOrderAsc, kOrderDesc; every other operator: kOrderIndex = 2


def assert_lists(got, want, flags=3):
    """(pass rows, order, lengths) of tas_eval against the oracle's, lists up to their length."""
    if flags & 1:
        np.testing.assert_array_equal(got[0], want[0])
    if flags & 2:
        np.testing.assert_array_equal(got[2], want[2])
        for p in range(len(want[2])):
            np.testing.assert_array_equal(got[1][p, :want[2][p]], want[1][p, :want[2][p]],
                                          err_msg=f"pod {p}")


def buckets(prio, present, m):
    """The grouping bucket of every pod as group_body computes it: order * M + metric, or 3 M
    (no list) for a metric out of range or one that no node reports."""
    cnt = unpack_bits(present, present.shape[1] * 64).sum(1)
    out = np.full(len(prio), 3 * m)
    for p, (metric, op, _) in enumerate(prio.tolist()):
        if 0 <= metric < m and cnt[metric] > 0:
            out[p] = ORDER_OF.get(op, 2) * m + metric
    return out


# ------------------------------------------------------------------ A. grouping: pods
@functools.lru_cache(maxsize=None)
def pods_case(p):
    """N = 130, M = 4, one snapshot for every pod count (the same seed draws it first)."""
    rng = np.random.default_rng(0xA0)
    v, pres, _, _, _, _ = random_case(rng, 130, 4, 1, 1)
    rng = np.random.default_rng(0xA0 + p)
    _, _, rules, off, prio, cand = random_case(rng, 130, 4, p, 3, cand_frac=0.8)
    b = buckets(prio, pres, 4)
    # all three orders and the no-list bucket G = 12 are populated
    assert set((b // 4).tolist()) == {0, 1, 2, 3}
    return v, pres, rules, off, prio, cand


@pytest.mark.parametrize("cand", [False, True])
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("p", [4096, 4097, 8193])
def test_grouping_rounds_by_pod_count(ctx, oracle, p, flags, cand):
    """group_body: `P <= kGroupTpb * kGU && M <= kGroupTpb` (P <= 4096, M <= 1024) is the
    register-resident single round.  P = 4096 is its last shape; P = 4097 is the first
    multi-round shape (keys scratch, a one-pod second round); P = 8193 is two full rounds and
    one pod."""
    v, pres, rules, off, prio, c = pods_case(p)
    assert_same(ctx, oracle, v, pres, rules, off, prio, c if cand else None, flags)


def test_grouping_multi_round_topk(ctx, oracle):
    """P = 4097 > kGroupTpb * kGU through pas_tas_topk_device (k = 5): the multi-round
    grouping under the top-k form of the eval, records against the first 5 oracle entries."""
    v, pres, rules, off, prio, cand = pods_case(4097)
    gen = upload(ctx, v, pres)
    P, k, base = 4097, 5, 1000
    _, order, lens = oracle.tas_eval(v, pres, rules, off, prio, cand, 3)
    batch = wl.TasBatch(rules, off, prio)
    key = torch.empty((P, k), dtype=torch.int64, device="cuda")
    node = torch.empty((P, k), dtype=torch.int32, device="cuda")
    ln = torch.empty(P, dtype=torch.int32, device="cuda")
    ctx.tas_topk_device(gen, P, len(rules), *_rule_tensors(batch, cand), k, base, key, node, ln)
    ctx.synchronize()
    want_k, want_n, want_l = narrow_records(v, prio, order, lens, k, base)
    np.testing.assert_array_equal(ln.cpu().numpy(), want_l)
    np.testing.assert_array_equal(node.cpu().numpy(), want_n)
    np.testing.assert_array_equal(key.cpu().numpy(), want_k)


def narrow_records(v, prio, order, lens, k, base):
    """The 64-bit records (pas.h) of the first k entries of the oracle's lists."""
    P = len(prio)
    keys = np.full((P, k), I64_MAX, np.int64)
    nodes = np.full((P, k), I32_MAX, np.int32)
    ln = np.minimum(lens, k).astype(np.int32)
    for p in np.nonzero(ln)[0]:  # (an empty list's metric may be out of range)
        loc = order[p, :ln[p]].astype(np.int64)
        nodes[p, :ln[p]] = loc + base
        keys[p, :ln[p]] = order_keys(v, prio, loc, p)
    return keys, nodes, ln


# ------------------------------------------------------------------ A. grouping: metrics
@functools.lru_cache(maxsize=None)
def metrics_case(m):
    n, p = (70, 64) if m == 4096 else (130, 300)
    rng = np.random.default_rng(0xB0 + m)
    v, pres, rules, off, prio, cand = random_case(rng, n, m, p, 3, cand_frac=0.8)
    # buckets 0, M - 2, 2 M + M - 2 and 3 M: metric 0 ascending, metric M - 2 ascending and in
    # index order, and the all-absent last column (cnt == 0: no list); M - 2 descending too
    forced = [(0, LT), (m - 2, LT), (m - 2, 3), (m - 1, GT), (m - 2, GT), (0, EQ), (m - 1, LT)]
    for i, (metric, op) in enumerate(forced * 3):
        prio[i] = (metric, op, 0)
    pb = unpack_bits(pres, n)
    pb[0, :3] = pb[m - 2, :3] = True  # (the two forced columns have nodes, whatever was drawn)
    pres = pack_bits(pb)
    b = buckets(prio, pres, m)
    assert {0, m - 2, 2 * m + m - 2, 3 * m, m + m - 2} <= set(b.tolist())
    assert not pb[m - 1].any() and (b[[3, 6]] == 3 * m).all()
    return v, pres, rules, off, prio, cand


@pytest.mark.parametrize("m", [1024, 1025, 4096])
def test_grouping_by_metric_count(ctx, oracle, m):
    """group_body: M = 1024 = kGroupTpb is the last metric count of the single round (the
    `cnt` table staged in LDS by one thread per metric); M = 1025 takes the multi-round path at
    P = 300 (`cnt` read from global memory, the scan over 3 M + 1 buckets); M = 4096 =
    kMaxGroupMetrics is the one accepted value whose group_lds (4 (4 M + 1) bytes) passes
    64 KiB, so prep_launch raises the kernel's dynamic LDS limit."""
    v, pres, rules, off, prio, cand = metrics_case(m)
    gen = upload(ctx, v, pres)
    for c in (cand, None):
        want = oracle.tas_eval(v, pres, rules, off, prio, c, 3)
        assert_lists(ctx.tas_eval(gen, rules, off, prio, c, 3), want)
    assert (want[2] > 0).mean() > 0.5


def test_metric_count_past_capacity(ctx, oracle):
    """M = 4097 > kMaxGroupMetrics: the snapshot is accepted, pas_tas_eval refuses it with
    PAS_ECAPACITY before any launch, the deschedule sweep still runs on it, and the context
    evaluates a following small snapshot."""
    rng = np.random.default_rng(0xC0)
    v, pres, rules, off, prio, _ = random_case(rng, 70, 4097, 16, 3)
    gen = upload(ctx, v, pres)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_eval(gen, rules, off, prio)
    assert e.value.code == _lib.PAS_ECAPACITY
    np.testing.assert_array_equal(ctx.tas_violations(gen, rules, off),
                                  oracle.tas_violations(v, pres, rules, off))
    v, pres, rules, off, prio, cand = random_case(rng, 130, 4, 9, 3, cand_frac=0.8)
    assert_same(ctx, oracle, v, pres, rules, off, prio, cand, 3)


# ------------------------------------------------------------------ B. global pass, chunked
GPASS = [(13, 5), (20, 9), (16, 16)]


@functools.lru_cache(maxsize=None)
def gpass_case(n, p):
    rng = np.random.default_rng(0xD0 + n + p)
    return random_case(rng, n, 4, p, 5, cand_frac=0.6)


@pytest.mark.parametrize("cand", [False, True])
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("n", [65, 1025])
@pytest.mark.parametrize("p,cap", GPASS)
def test_global_pass_in_several_launches(ctx, oracle, monkeypatch, p, cap, n, flags, cand):
    """tas_eval_launch, global_pass: `for (p0 = 0; p0 < n_pods; p0 += chunk)` with
    pos_base = p0.  (P, cap) = (13, 5): grids of 5, 5 and 3 blocks, all below 8, so
    per_xcd == 0 in the XCD slot formula; (20, 9): grids of 9 (per_xcd = 1, rem = 1), 9 and a
    2-block tail; (16, 16): one launch, the control."""
    monkeypatch.setenv("PAS_EVAL_GLOBAL_PASS", "1")
    monkeypatch.setenv("PAS_EVAL_GPASS_PODS", str(cap))
    v, pres, rules, off, prio, c = gpass_case(n, p)
    assert_same(ctx, oracle, v, pres, rules, off, prio, c if cand else None, flags)


def test_global_pass_slot_buffer_per_stream(oracle, monkeypatch):
    """The stream's kBufGpass slot buffer holds `chunk` bitmap rows, not n_pods: on a fresh
    context, (P, cap) = (13, 5) on one stream, then (20, 9) on a second stream (its own slot,
    9 rows) and again on the first (whose buffer of 5 rows has to grow)."""
    monkeypatch.setenv("PAS_EVAL_GLOBAL_PASS", "1")
    n = 1025
    v, pres, _, _, _, _ = gpass_case(n, 13)
    with pas_amd.Context(0) as c:
        c.tas_snapshot_set(1, v, pres)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for (p, cap), st in (((13, 5), streams[0]), ((20, 9), streams[1]), ((20, 9), streams[0])):
            monkeypatch.setenv("PAS_EVAL_GPASS_PODS", str(cap))
            _, _, rules, off, prio, cand = gpass_case(n, p)
            with torch.cuda.stream(st):
                t = _rule_tensors(wl.TasBatch(rules, off, prio), cand)
                pt = torch.empty((p, pas_amd.w64(n)), dtype=torch.int64, device="cuda")
                ot = torch.empty((p, n), dtype=torch.int32, device="cuda")
                lt = torch.empty(p, dtype=torch.int32, device="cuda")
            st.synchronize()  # (the inputs are there before the library's stream reads them)
            c.tas_eval_device(1, p, len(rules), *t, 3, pt, ot, lt, st)
            st.synchronize()
            got = (pt.cpu().numpy().view(np.uint64), ot.cpu().numpy(), lt.cpu().numpy())
            assert_lists(got, oracle.tas_eval(v, pres, rules, off, prio, cand, 3))


# ------------------------------------------------------------------ C. top-k past 16 cards
TN, TP, TM, TBASE = 700, 40, 5, 1234


@functools.lru_cache(maxsize=None)
def cards_case(oracle, K):
    """N = 700 nodes of up to K cards (Q = 3, per-GPU i915 capacity 1..4), 40 pods of up to 8
    selections.  On four nodes of five the i915 shares of cards 0..15 are used up, so a pod
    that fits there fits on the cards past 16.  TAS: 5 milli columns of few distinct values;
    column 1 is also given wide (whole, nano) for the wide entry points."""
    rng = np.random.default_rng(0xE0 + K)
    n_cards, cap, used, req, mask, ncont = random_wide(rng, TN, K, 3, TP, 3, 8)
    full = rng.random(TN) < 0.8
    used[full, :16, 0] = cap[full, 0][:, None]
    gs, gb = wl.GasSnapshotData(n_cards, cap, used), wl.GasBatch(req, mask, ncont)
    words, sel, nsel = oracle.gas_fit(n_cards, cap, used, req, mask, ncont, 0, selections=True)
    fits = (words >> 31).astype(bool)
    high = (sel >= 16) & (np.arange(sel.shape[2]) < nsel[:, :, None])
    share = (high.any(2) & fits).sum() / fits.sum()
    assert fits.mean() > 0.1 and share >= 0.25, (fits.mean(), share)
    v = rng.integers(0, 12, (TM, TN)).astype(np.int64) * 1000
    whole = rng.integers(0, 12, TN).astype(np.int64)
    nano = rng.choice(np.array([0, 0, 1, 500_000_000, 999_999_999], np.uint32), TN)
    v[1] = whole * 1000 + nano.astype(np.int64) // 10**6  # (the narrow snapshot's column 1)
    pres = pack_bits(rng.random((TM, TN)) < 0.95)
    n_r = rng.integers(0, 3, TP)
    off = np.concatenate([[0], np.cumsum(n_r)]).astype(np.int32)
    rules = np.zeros(int(off[-1]), RULE_DTYPE)
    rules["metric"] = rng.integers(-1, TM + 1, len(rules))
    rules["op"] = rng.integers(0, 3, len(rules))
    rules["target"] = rng.integers(-1, 13, len(rules))
    rules["target"][rules["op"] == LT] = rng.integers(-1, 4, (rules["op"] == LT).sum())
    rules["target"][rules["op"] == GT] = rng.integers(8, 13, (rules["op"] == GT).sum())
    prio = np.zeros(TP, RULE_DTYPE)
    prio["metric"] = np.where(np.arange(TP) % 2 == 0, 1, rng.integers(0, TM, TP))
    prio["op"] = np.array([GT, LT, EQ, 7])[(np.arange(TP) // 2) % 4]
    prio["metric"][TP - 1] = TM  # no scheduling rule: empty list
    cand = pack_bits(rng.random((TP, TN)) < 0.8)
    for a in (v, pres, rules, off, prio, cand):
        a.setflags(write=False)
    narrow = dict(v=v, pres=pres, rules=rules, off=off, prio=prio, gs=gs, gb=gb, i915=0,
                  scale=[3] * TM, wide={})
    return narrow, dict(narrow, wide={1: (whole, nano)}), cand, fits


@functools.lru_cache(maxsize=None)
def cards_expected(oracle, K, wide, with_cand):
    """Every pod's whole list of records (k = N) by the oracle composition: oracle.gas_fit's
    fit bits and the candidates -> oracle.tas_eval -> records.  (key, [sub,] node, len)."""
    narrow, held_wide, cand, fits = cards_case(oracle, K)
    cand = cand if with_cand else None
    if wide:
        return c5_expected(oracle, held_wide, cand, TN, TBASE)
    ok = fits & unpack_bits(cand, TN) if with_cand else fits
    _, order, lens = oracle.tas_eval(narrow["v"], narrow["pres"], narrow["rules"], narrow["off"],
                                     narrow["prio"], pack_bits(ok), 3)
    return narrow_records(narrow["v"], narrow["prio"], order, lens, TN, TBASE)


def cards_dev(ctx, oracle, K, wide, with_cand):
    narrow, held_wide, cand, _ = cards_case(oracle, K)
    c = dict(held_wide if wide else narrow, cand=cand if with_cand else None)
    return Dev(ctx, c, scale=c["scale"], wide=c["wide"])


def first_k(full, k):
    """The records of the first k entries of whole lists, padded as a k-wide call pads them."""
    *arrays, ln = full
    return tuple(a[:, :k] for a in arrays) + (np.minimum(ln, k),)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("k", [1, 16])
@pytest.mark.parametrize("K", [17, 64])
def test_topk_past_16_cards(ctx, oracle, K, k, wide):
    """topk_dispatch: neither `a.K <= 8` nor `a.K <= 16`, so the
    <PAS_GAS_MAX_CARDS, kMaxRes, kWide, false> instantiation (card copy in scratch, not
    unrolled).  K = 17 is the first such width, K = 64 the widest; pas_tas_gas_topk_device and,
    on a snapshot with one wide column, pas_tas_gas_topk_wide_device."""
    with_cand = (K == 17) == (k == 1)
    dev = cards_dev(ctx, oracle, K, wide, with_cand)
    assert ctx.gas_snapshot_info()[2] == K and ctx.tas_snapshot_wide_count() == int(wide)
    got = dev.topk(k, TBASE, wide=wide)
    want = first_k(cards_expected(oracle, K, wide, with_cand), k)
    for g, w, name in zip(got, want, ("key", "sub", "node", "len") if wide else
                          ("key", "node", "len")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert (want[-1] == k).mean() > 0.5 and want[-1][TP - 1] == 0


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("K", [17, 64])
def test_topk_after_past_16_cards(ctx, oracle, K, wide):
    """topk_dispatch's last tier with kAfter: <PAS_GAS_MAX_CARDS, kMaxRes, kWide, true>.
    Pages of k = 7 from the begin cursor until every list is exhausted; their concatenation
    is the oracle composition's whole list."""
    k = 7
    with_cand = (K == 64) == wide
    dev = cards_dev(ctx, oracle, K, wide, with_cand)
    *want, L = cards_expected(oracle, K, wide, with_cand)
    assert (L > 2 * k).mean() > 0.5
    # (past a list's end a page holds the padding record)
    want = [np.hstack([w, np.full((TP, 2 * k), np.iinfo(w.dtype).max, w.dtype)]) for w in want]
    cur = (np.full(TP, I64_MIN),) + ((np.zeros(TP, np.uint32),) if wide else ()) + \
        (np.full(TP, -1),)
    for i in range(TN // k + 2):
        page = dev.topk(k, TBASE, after=cur, wide=wide)
        np.testing.assert_array_equal(page[-1], np.clip(L - i * k, 0, k), f"page {i} len")
        for got, w in zip(page[:-1], want):
            np.testing.assert_array_equal(got, w[:, i * k:(i + 1) * k], f"page {i}")
        if not page[-1].any():
            break
        cur = last_record(page, k)
    else:
        pytest.fail("the lists were not exhausted")


# ------------------------------------------------------------------ D. node-major copies
def copy_bytes(n, m):
    """(vals_t, pres_t) allocation sizes of tas_gas_topk_launch for an [n][m] snapshot."""
    return 8 * n * m, 8 * n * ((m + 63) // 64)


def pres_growing_pair():
    """The first shape pair (from 20 nodes up) with equal byte sums where N grows, M drops and
    only pres_t grows."""
    shapes = ((a, b, c, d) for a in range(20, 40) for b in range(65, 200)
              for c in range(a + 1, 80) for d in range(1, b))
    return next(((a, b), (c, d)) for a, b, c, d in shapes
                if sum(copy_bytes(a, b)) == sum(copy_bytes(c, d))
                and copy_bytes(c, d)[1] > copy_bytes(a, b)[1])


def tas_content(rng, n, m):
    v = rng.integers(0, 9, (m, n)).astype(np.int64) * 1000
    return v, rng.random((m, n)) < 0.9


def gas_content(rng, n):
    gs = wl.make_gas_snapshot(n, seed=int(rng.integers(1, 1 << 30)), no_label_frac=0.0)
    return gs.n_cards, gs.cap, gs.used


def copies_batch(rng, m, P=24):
    off = np.arange(P + 1, dtype=np.int32)
    rules = np.zeros(P, RULE_DTYPE)
    rules["metric"] = rng.integers(0, m, P)
    rules["op"] = rng.integers(0, 3, P)
    rules["target"] = rng.integers(0, 9, P)
    prio = np.zeros(P, RULE_DTYPE)
    prio["metric"] = rng.integers(0, m, P)
    prio["op"] = rng.integers(0, 4, P)
    return wl.TasBatch(rules, off, prio), wl.make_gas_batch(P, seed=int(rng.integers(1, 1 << 30)))


def lazy_topk(c, gens, batch, gb, k):
    P = len(batch.prio)
    key = torch.empty((P, k), dtype=torch.int64, device="cuda")
    node = torch.empty((P, k), dtype=torch.int32, device="cuda")
    ln = torch.empty(P, dtype=torch.int32, device="cuda")
    c.tas_gas_topk_device(*gens, P, len(batch.rules), *_rule_tensors(batch, None),
                          gb.req.shape[1], wl.I915, _dev(gb.req),
                          _dev(gb.req_mask.view(np.int32)), _dev(gb.n_containers), k, 0, key,
                          node, ln)
    c.synchronize()
    return key.cpu().numpy(), node.cpu().numpy(), ln.cpu().numpy()


def composition(oracle, v, pb, gas, batch, gb, k):
    fit = (oracle.gas_fit(*gas, gb.req, gb.req_mask, gb.n_containers, wl.I915) >> 31).astype(bool)
    _, order, lens = oracle.tas_eval(v, pack_bits(pb), batch.rules, batch.rule_off, batch.prio,
                                     pack_bits(fit), 3)
    return narrow_records(v, batch.prio, order, lens, k, 0)


def assert_records(got, want, what):
    for g, w, name in zip(got, want, ("key", "node", "len")):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


@functools.lru_cache(maxsize=None)
def copy_plan(oracle, small, big):
    """The inputs of run_copy_sequence and the oracle compositions of its two states."""
    (n0, m0), (n1, m1) = small, big
    rng = np.random.default_rng(n0 * 1000 + m0)
    k = 6
    v0, pb0 = tas_content(rng, n0, m0)
    g0 = gas_content(rng, n0)
    b0, gb = copies_batch(rng, m0)
    src = rng.permutation(m0)[:m1].astype(np.int32)
    g_new = gas_content(rng, n1 - n0)
    v1 = np.zeros((m1, n1), np.int64)
    pb1 = np.zeros((m1, n1), bool)
    v1[:, :n0], pb1[:, :n0] = v0[src], pb0[src]
    cols = np.arange(0, m1, max(m1 // 8, 1))
    nv, npb = tas_content(rng, n1, len(cols))
    v1[cols], pb1[cols] = nv, npb
    g1 = (np.concatenate([g0[0], g_new[0]]), np.concatenate([g0[1], g_new[1]]),
          np.concatenate([g0[2], np.zeros_like(g_new[2])]))
    b1, _ = copies_batch(rng, m1)
    b1.prio["metric"][:len(cols)] = cols  # (lists that hold the new nodes)
    want0 = composition(oracle, v0, pb0, g0, b0, gb, k)
    want1 = composition(oracle, v1, pb1, g1, b1, gb, k)
    assert (want0[2] > 0).mean() > 0.5 and (want1[1][want1[1] != I32_MAX] >= n0).any()
    return dict(k=k, v0=v0, pb0=pb0, g0=g0, b0=b0, gb=gb, src=src, g_new=g_new, v1=v1, pb1=pb1,
                cols=cols, nv=nv, npb=npb, g1=g1, b1=b1, want0=want0, want1=want1)


def run_copy_sequence(oracle, small, big):
    """(n0, m0) resident and evaluated, reshaped to (n1, m1) with the GAS snapshot resized and
    the new nodes filled, evaluated; then a snapshot_set back to (n0, m0), evaluated."""
    (n0, m0), (n1, m1) = small, big
    q = copy_plan(oracle, small, big)
    k, gb, K = q["k"], q["gb"], q["g0"][2].shape[1]
    with pas_amd.Context(0) as c:
        # 1, 2: the copies are allocated for (n0, m0)
        c.tas_snapshot_set(10, q["v0"], pack_bits(q["pb0"]))
        c.gas_snapshot_set(11, *q["g0"])
        assert_records(lazy_topk(c, (10, 11), q["b0"], gb, k), q["want0"], "before the reshape")
        # 3: both snapshots to n1 nodes, m1 of the old columns in a shuffled order
        c.gas_snapshot_resize(11, 12, n1, K)
        st = c.gas_nodes_update(12, 13, np.arange(n0, n1), q["g_new"][0], q["g_new"][1],
                                np.full((n1 - n0, K), -1, np.int32))
        assert not st.any()
        c.tas_snapshot_reshape(10, 20, n1, m1, q["src"])
        # 4: a few columns updated, so that the new nodes carry values
        c.tas_snapshot_update(20, 21, q["cols"], q["nv"], pack_bits(q["npb"]))
        # 5: against a second fresh context given the final matrices, and the oracle
        got = lazy_topk(c, (21, 13), q["b1"], gb, k)
        with pas_amd.Context(0) as c2:
            c2.tas_snapshot_set(1, q["v1"], pack_bits(q["pb1"]))
            c2.gas_snapshot_set(2, *q["g1"])
            assert_records(got, lazy_topk(c2, (1, 2), q["b1"], gb, k),
                           "after the reshape, against the direct snapshot")
        assert_records(got, q["want1"], "after the reshape")
        # back through pas_tas_snapshot_set (free_tas: the copies are dropped and rebuilt)
        c.tas_snapshot_set(30, q["v0"], pack_bits(q["pb0"]))
        c.gas_snapshot_set(31, *q["g0"])
        assert_records(lazy_topk(c, (30, 31), q["b0"], gb, k), q["want0"], "after the set back")


def test_copies_across_reshape_vals_grow(oracle):
    """tas_gas_topk_launch re-allocates the node-major copies when either is too small.
    (N, M) = (25, 166) -> (65, 64): the two sizes' sum stays 33 800 bytes while vals_t grows
    from 33 200 to 33 280, which a compare of the sum (the reshape carries the sizes over)
    does not see.  Then the shapes swapped: (65, 64) resident, a set of (25, 166)."""
    small, big = (25, 166), (65, 64)
    (v0, p0), (v1, p1) = copy_bytes(*small), copy_bytes(*big)
    assert v0 + p0 == v1 + p1 == 33800 and (v0, v1) == (33200, 33280)
    run_copy_sequence(oracle, small, big)


def test_copies_across_reshape_pres_grows(oracle):
    """The same sequence on the first pair of equal sums where only pres_t grows: pres_t was
    allocated for fewer (node, 64-column word) pairs than the reshaped snapshot has."""
    small, big = pres_growing_pair()
    (v0, p0), (v1, p1) = copy_bytes(*small), copy_bytes(*big)
    assert v0 + p0 == v1 + p1 and p1 > p0 and v1 < v0 and big[0] > small[0] and big[1] < small[1]
    run_copy_sequence(oracle, small, big)
