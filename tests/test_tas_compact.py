"""pas_tas_snapshot_compact: node slots dropped and renumbered on the device.

The checker is test_tas_reshape.py's (its Content / probe / answers helpers are copied here):
the from-scratch build of the host-compacted content on a later generation of the session
context, pas_tas_snapshot_set + pas_tas_snapshot_set_scale + pas_tas_snapshot_update_wide
(Context.tas_snapshot_set_wide), then the same calls.  Every answer is compared bit for bit.

Columns (M = 5): milli at about 70 % presence, scale 6 with few distinct values and every node
present (tie order), wide, empty, signed milli.  The node shapes are the smallest at which each
hazard exists:
  130 -> 100 (random 30 dropped)   W64 3 -> 2: the new sentinel 128 is below old live ids
  1100 -> 1000, 1025 -> 1024       R 3072 -> 2048: row pitch, fence pitch, plane stride
  2500 -> about 1750               several segments per order row with drops in each: the
                                   scan's bases
  2600 -> 2048                     cnt' of the fully present column lands on a 1024 and a 32
                                   boundary
  70 -> 70 spare slots, 70 -> 0    every column empties
  identity, identity + -1 tail     the generation alone; the reshape's growth
  -1 entries in the middle         spare gaps
  the present nodes of column 0    that column's cnt' becomes 0 while others keep entries
  stale upload bits                bits past n_nodes in the last presence word never become
                                   nodes
A snapshot of zero nodes has nothing to evaluate: that case compares pas_tas_snapshot_get, then
grows both sides back to 70 slots (the reshape's tested 0 -> 70) and compares the answers
there, which read the compaction's cnt'."""
import itertools

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd.workload import pack_bits, unpack_bits
from helpers import RULE_DTYPE

TARGETS = [2, 5, 10**16]
M = 5
_gen = itertools.count(0x7C60000, 16)


def pack(b):
    """pack_bits, also for no rows or no nodes."""
    b = np.asarray(b, bool)
    if b.size:
        return pack_bits(b)
    return np.zeros(b.shape[:-1] + ((b.shape[-1] + 63) // 64,), np.uint64)


class Content:
    """What a snapshot holds: v [M][N] at the columns' scales (floors for a wide column),
    pres [M][N] bool, scale [M], wide {m: nano [N]}."""

    def __init__(self, v, pres, scale, wide):
        self.v, self.pres, self.scale, self.wide = v, pres, scale, wide
        self.M, self.N = v.shape

    def install(self, ctx, gen, stale=False):
        p = pack(self.pres)
        if stale:  # the upload's last word carries bits past n_nodes
            assert self.N % 64
            p[:, -1] |= np.uint64(~((1 << (self.N % 64)) - 1) & (2**64 - 1))
        ctx.tas_snapshot_set_wide(gen, self.v, p, self.scale,
                                  {m: (self.v[m], f) for m, f in self.wide.items()})

    def compacted(self, src):
        """The host compaction: new slot j holds old slot src[j], or nothing for -1."""
        src = np.asarray(src, np.int64).reshape(-1)
        keep = src >= 0
        at = np.where(keep, src, 0)
        if self.N == 0:  # (nothing to gather from)
            at = np.zeros(0, np.int64)
            assert not keep.any()
        v = np.zeros((self.M, len(src)), np.int64)
        pres = np.zeros((self.M, len(src)), bool)
        wide = {}
        if len(at):
            v = np.where(keep, self.v[:, at], 0)
            pres = np.where(keep, self.pres[:, at], False)
            wide = {m: np.where(keep, f[at], 0).astype(np.uint32) for m, f in self.wide.items()}
        else:
            wide = {m: np.zeros(len(src), np.uint32) for m in self.wide}
        return Content(v, pres, self.scale.copy(), wide)

    def grown(self, n1):
        """Spare slots appended (the reshape's growth)."""
        return self.compacted(list(range(self.N)) + [-1] * (n1 - self.N))


def make_content(seed, n, m=M):
    rng = np.random.default_rng(seed)
    v = np.zeros((m, n), np.int64)
    pres = np.zeros((m, n), bool)
    scale = np.full(m, 3, np.int32)
    wide = {}
    for c in range(m):
        kind = c % 5
        pres[c] = rng.random(n) < 0.7
        if kind == 0:  # milli
            v[c] = rng.integers(0, 10, n) * 1000
        elif kind == 1:  # scale 6, few distinct values: ties; every node present
            scale[c] = 6
            v[c] = rng.integers(0, 6, n) * 10**6 + rng.choice([0, 1, 500000], n)
            pres[c] = True
        elif kind == 2:  # wide
            v[c] = rng.choice(list(range(10)) + [10**16, 10**16 + 1, -3], n)
            wide[c] = rng.choice([0, 1, 999999999], n).astype(np.uint32)
        elif kind == 3:  # empty
            pres[c] = False
        else:
            v[c] = rng.integers(-5, 5, n) * 1000
    return Content(v, pres, scale, wide)


def probe(m):
    """Single-rule pods: every (column, operator, target), one rule on an unknown metric; the
    prioritize rules walk every (column, operator)."""
    trip = [(c, op, t) for c in range(m) for op in range(3) for t in TARGETS] + [(-1, 0, 0)]
    rules = np.array(trip, RULE_DTYPE)
    off = np.arange(len(trip) + 1, dtype=np.int32)
    prio = np.zeros(len(trip), RULE_DTYPE)
    for i in range(len(trip)):
        prio[i] = (i % m, (i // m) % 3, 0) if m else (-1, 0, 0)
    return rules, off, prio


def answers(ctx, gen, n, m=M):
    """Every answer the tests compare, as plain lists."""
    import torch
    rules, off, prio = probe(m)
    P = len(prio)
    out = []
    gp, go, gl = ctx.tas_eval(gen, rules, off, prio)
    out.append(gp.tolist())
    out.append([go[p, :gl[p]].tolist() for p in range(P)])
    out.append(ctx.tas_violations(gen, rules, off).tolist())
    rng = np.random.default_rng(5)
    req = np.concatenate([rng.permutation(n), [-1], np.arange(n)[: n // 3]]).astype(np.int32)
    for c, op in itertools.product(range(m), range(3)):
        out.append(ctx.tas_prioritize_request(gen, (c, op, 0), req).tolist())
    k = 4
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    key = torch.zeros((P, k), dtype=torch.int64, device="cuda")
    sub = torch.zeros((P, k), dtype=torch.int32, device="cuda")
    node = torch.zeros((P, k), dtype=torch.int32, device="cuda")
    ln = torch.zeros(P, dtype=torch.int32, device="cuda")
    ctx.tas_topk_wide_device(gen, P, len(rules), dev(rules.view(np.uint8)), dev(off),
                             dev(prio.view(np.uint8)), None, k, 0, key, sub, node, ln,
                             stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    ln = ln.cpu().numpy()
    for t in (key, sub, node):
        a = t.cpu().numpy()
        out.append([a[p, :ln[p]].tolist() for p in range(P)])
    return out


def snapshot(ctx):
    """pas_tas_snapshot_get with the values and nanos of absent nodes zeroed (they are
    meaningful only where the bit is set), as plain lists, without the generation."""
    _, vals, present, scale, wide, nano = ctx.tas_snapshot_get()
    pres = unpack_bits(present, vals.shape[1]) if vals.size else np.zeros(vals.shape, bool)
    return [np.where(pres, vals, 0).tolist(), present.tolist(), scale.tolist(), wide.tolist(),
            np.where(pres, nano, 0).tolist()]


def check_get(ctx, gen, c):
    g, vals, present, scale, wide, nano = ctx.tas_snapshot_get()
    assert g == gen and vals.shape == (c.M, c.N)
    np.testing.assert_array_equal(present, pack(c.pres))  # and no bit past N
    np.testing.assert_array_equal(np.where(c.pres, vals, 0), np.where(c.pres, c.v, 0))
    np.testing.assert_array_equal(scale, c.scale)
    assert [int(x) for x in wide] == [int(m in c.wide) for m in range(c.M)]
    for m in range(c.M):
        want = c.wide[m] if m in c.wide else np.zeros(c.N, np.uint32)
        np.testing.assert_array_equal(np.where(c.pres[m], nano[m], 0), np.where(c.pres[m], want, 0))


def drop_random(n, n_drop, seed):
    return np.sort(np.random.default_rng(seed).permutation(n)[n_drop:]).tolist()


def with_gaps(src, every):
    """A -1 before every `every`-th entry of src."""
    out = []
    for i, s in enumerate(src):
        if i % every == every - 1:
            out.append(-1)
        out.append(s)
    return out


def case_map(name, c):
    """(src_node, stale upload) of a named case on content c."""
    n = c.N
    if name == "drop30":
        return drop_random(n, 30, 1), False
    if name == "drop100":
        return drop_random(n, 100, 2), False
    if name == "drop1":
        return drop_random(n, 1, 3), False
    if name == "drop30pct":
        return np.flatnonzero(np.random.default_rng(4).random(n) >= 0.3).tolist(), False
    if name == "to2048":
        return drop_random(n, n - 2048, 5), False
    if name == "all_spare":
        return [-1] * n, False
    if name == "none":
        return [], False
    if name == "identity":
        return list(range(n)), False
    if name == "identity_tail":
        return list(range(n)) + [-1] * 40, False
    if name == "gaps":
        return with_gaps(drop_random(n, 20, 6), 7), False
    if name == "column0":
        return np.flatnonzero(~c.pres[0]).tolist(), False
    if name == "stale":
        return with_gaps(drop_random(n, 30, 7), 9), True
    raise KeyError(name)


CASES = [(130, "drop30"), (1100, "drop100"), (1025, "drop1"), (2500, "drop30pct"),
         (2600, "to2048"), (70, "all_spare"), (70, "none"), (130, "identity"),
         (130, "identity_tail"), (1100, "gaps"), (1100, "column0"), (130, "stale")]


@pytest.mark.gpu
@pytest.mark.parametrize("n0,name", CASES)
def test_compact_equals_from_scratch(ctx, n0, name):
    gen = next(_gen)
    c0 = make_content(n0 * 7 + 1, n0)
    src, stale = case_map(name, c0)
    n1 = len(src)
    c0.install(ctx, gen, stale=stale)
    ctx.tas_snapshot_compact(gen, gen + 1, src)
    assert ctx.tas_snapshot_info() == (gen + 1, n1, M)
    c1 = c0.compacted(src)
    if name == "to2048":
        assert c1.pres[1].sum() == 2048
    if name == "column0":
        assert c1.pres[0].sum() == 0 and c1.pres[1].sum() > 0 and c1.pres[4].sum() > 0
    check_get(ctx, gen + 1, c1)
    assert ctx.tas_snapshot_wide_count() == len(c1.wide)
    state = snapshot(ctx)
    g = gen + 1
    if n1 == 0:  # nothing to evaluate over no nodes: the answers of both sides grown to 70
        ctx.tas_snapshot_reshape(g, g + 1, 70, M)
        g, n1 = g + 1, 70
    got = answers(ctx, g, n1)
    # the checker: the same content from scratch
    c1.install(ctx, gen + 8)
    assert snapshot(ctx) == state
    if c1.N == 0:
        c1.grown(70).install(ctx, gen + 8)
    assert answers(ctx, gen + 8, n1) == got


@pytest.mark.gpu
def test_compact_then_updates(ctx):
    """The new storage's build scratch is usable: a narrow update of one column and a wide
    update of another on the new shape, against the same updates on the from-scratch build."""
    gen = next(_gen)
    c0 = make_content(77, 1100)
    src = with_gaps(drop_random(1100, 100, 8), 50)
    n1 = len(src)
    c0.install(ctx, gen)
    ctx.tas_snapshot_compact(gen, gen + 1, src)

    def refresh(g, c):
        rng = np.random.default_rng(9)
        v, p = rng.integers(0, 10, n1) * 1000, rng.random(n1) < 0.7
        ctx.tas_snapshot_update(g, g + 1, [0], v[None, :], pack_bits(p[None, :]))
        c.v[0], c.pres[0] = v, p
        w, pw = rng.integers(0, 10, n1), rng.random(n1) < 0.7
        f = rng.choice([0, 7], n1).astype(np.uint32)
        ctx.tas_snapshot_update_wide(g + 1, g + 2, [3], w[None, :], f[None, :],
                                     pack_bits(pw[None, :]))
        c.v[3], c.pres[3], c.wide[3] = w, pw, f
        return g + 2

    c1 = c0.compacted(src)
    g = refresh(gen + 1, c1)
    check_get(ctx, g, c1)
    got = answers(ctx, g, n1)
    c2 = c0.compacted(src)
    c2.install(ctx, gen + 8)
    g = refresh(gen + 8, c2)
    assert answers(ctx, g, n1) == got


@pytest.mark.gpu
def test_refusals_leave_the_snapshot(ctx):
    gen = next(_gen)
    c = make_content(3, 100)
    c.install(ctx, gen)
    base, state = answers(ctx, gen, 100), snapshot(ctx)
    inc = list(range(50))
    bad = [((gen + 1, gen + 2, inc), _lib.PAS_ESTALE),
           ((gen, gen + 1, [0, 2, 1]), _lib.PAS_EINVAL),        # not increasing
           ((gen, gen + 1, [0, 1, -1, 1]), _lib.PAS_EINVAL),    # a slot twice
           ((gen, gen + 1, [98, 99, 100]), _lib.PAS_EINVAL),    # >= n_nodes
           ((gen, gen + 1, [0, -2, 1]), _lib.PAS_EINVAL)]       # < -1
    for args, code in bad:
        with pytest.raises(pas_amd.PasError) as e:
            ctx.tas_snapshot_compact(*args)
        assert e.value.code == code, args
        ctx.n_nodes = 100  # (the handle's shape follows successful calls only)
        assert ctx.tas_snapshot_info() == (gen, 100, M)
        assert snapshot(ctx) == state
    assert answers(ctx, gen, 100) == base
    # no snapshot
    assert pas_amd.LIB.pas_tas_snapshot_drop(ctx._h) == _lib.PAS_OK
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_snapshot_compact(gen, gen + 1, inc)
    assert e.value.code == _lib.PAS_ENOSNAP
    ctx.n_nodes = 100


# ------------------------------------------------------------------ no GPU

def test_header_and_library_declare_the_calls():
    from ctypes import c_int, c_int32, c_uint64, c_void_p
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in ("pas_tas_snapshot_compact", "pas_gas_snapshot_compact"):
        assert f"int {name}(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to," in header
        fn = getattr(pas_amd.LIB, name)
        assert fn.restype == c_int
        assert fn.argtypes == [c_void_p, c_uint64, c_uint64, c_int32, c_void_p, c_void_p]
        assert fn.argtypes == _lib.SIGNATURES[name][1]
    for method in ("tas_snapshot_compact", "gas_snapshot_compact"):
        assert callable(getattr(pas_amd.Context, method))
    from pas_amd.gas_cache import GasCache
    from pas_amd.tas_cache import TasCache
    assert callable(TasCache.compact) and callable(GasCache.compact)


def test_abi_version_and_timing_ids_stay():
    assert pas_amd.LIB.pas_abi_version() == 3
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "#define PAS_K_COUNT 10" in header


def test_null_context_is_einval():
    assert pas_amd.LIB.pas_tas_snapshot_compact(None, 0, 0, 0, None, None) == _lib.PAS_EINVAL
    assert pas_amd.LIB.pas_gas_snapshot_compact(None, 0, 0, 0, None, None) == _lib.PAS_EINVAL
