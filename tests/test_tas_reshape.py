"""pas_tas_snapshot_reshape and pas_tas_snapshot_get.

The checker is always the from-scratch build of the same content on a later generation of the
session context: pas_tas_snapshot_set + pas_tas_snapshot_set_scale + pas_tas_snapshot_update_wide
(Context.tas_snapshot_set_wide), then the same calls.  Every answer is compared bit for bit.

The node shapes are the smallest at which each hazard exists:
  100 -> 130    W64 2 -> 3: the old sentinel 128 becomes a node id; R stays 2048
  1000 -> 1100  R 2048 -> 3072: row pitch, fence pitch and plane stride change
  1024 -> 1025  both at once
  64 -> 64      column changes only
  0 -> 70, and M 0 -> 2: empty starts
Columns (M = 3): milli at about 70 % presence, scale 6 with ties and every node present, wide
at about 70 %; the five-column cases add an empty column and a second milli column."""
import itertools

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd.workload import pack_bits, unpack_bits
from helpers import RULE_DTYPE

TARGETS = [2, 5, 10**16]
_gen = itertools.count(0x7A50000, 16)


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

    def reshaped(self, n1, m1, src):
        src = list(src) if src is not None else [m if m < self.M else -1 for m in range(m1)]
        v = np.zeros((m1, n1), np.int64)
        pres = np.zeros((m1, n1), bool)
        scale = np.full(m1, 3, np.int32)
        wide = {}
        for m, s in enumerate(src):
            if s >= 0:
                v[m, :self.N], pres[m, :self.N], scale[m] = self.v[s], self.pres[s], self.scale[s]
                if s in self.wide:
                    wide[m] = np.concatenate([self.wide[s], np.zeros(n1 - self.N, np.uint32)])
        return Content(v, pres, scale, wide)


def make_content(seed, n, m):
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


def answers(ctx, gen, n, m):
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
    if m == 0:  # no column to order by
        return out
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


def refresh_plan(c, n_old, seed):
    """One narrow update of a kept column and one wide update of an added column (where the
    content has them), a new node (where there is one) holding the least value of each."""
    rng = np.random.default_rng(seed)
    new_node = n_old if c.N > n_old else None

    def column():
        v = rng.integers(0, 10, c.N) * 1000
        p = rng.random(c.N) < 0.7
        if new_node is not None:
            v[new_node], p[new_node] = -7000, True
        return v, p

    plan = []
    kept = next((m for m in range(c.M) if c.pres[m].any()), None)
    if kept is not None:
        plan.append(("narrow", kept) + column())
    added = next((m for m in range(c.M) if not c.pres[m].any() and m != kept), None)
    if added is not None:
        v, p = column()
        plan.append(("wide", added, v // 1000, p, rng.choice([0, 7], c.N).astype(np.uint32)))
    return plan, new_node


def apply_refresh(ctx, gen, c, plan):
    """The plan's calls on the context, and the same on the content; the last generation."""
    for step in plan:
        kind, m, v, p = step[:4]
        c.v[m], c.pres[m] = v, p
        pw = pack_bits(p[None, :])
        if kind == "narrow":
            ctx.tas_snapshot_update(gen, gen + 1, [m], v[None, :], pw)
            c.wide.pop(m, None)
        else:
            ctx.tas_snapshot_update_wide(gen, gen + 1, [m], v[None, :], step[4][None, :], pw)
            c.wide[m] = step[4]
        gen += 1
    return gen


SHAPES = [(100, 130), (1000, 1100), (1024, 1025), (64, 64)]
MAPS = {"add2": (None, 5), "drop_mid": ([0, 2], 2), "reverse": ([2, 1, 0], 3),
        "drop_all": ([], 0)}
CASES = [(n0, n1, 3, src, m1) for (n0, n1) in SHAPES for src, m1 in MAPS.values()]
CASES += [(n0, n1, 3, None, 3) for (n0, n1) in SHAPES[:3]]  # growth alone
CASES += [(1024, 1025, 5, [4, 3, 2, 1, 0], 5), (1000, 1100, 5, [0, 1, -1, 3, 4, 2], 6),
          (0, 70, 3, None, 3), (0, 70, 3, [2, -1, 0], 3), (100, 130, 0, None, 2),
          (64, 64, 0, None, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("n0,n1,m0,src,m1", CASES)
def test_reshape_equals_from_scratch(ctx, n0, n1, m0, src, m1):
    gen = next(_gen)
    c0 = make_content(n0 * 7 + m0, n0, m0)
    stale = n0 == 100
    c0.install(ctx, gen, stale=stale)
    ctx.tas_snapshot_reshape(gen, gen + 1, n1, m1, src)
    assert ctx.tas_snapshot_info() == (gen + 1, n1, m1)
    c1 = c0.reshaped(n1, m1, src)
    check_get(ctx, gen + 1, c1)
    assert ctx.tas_snapshot_wide_count() == len(c1.wide)
    got = answers(ctx, gen + 1, n1, m1)
    if stale:  # slots 100 .. 129 were upload bits past n_nodes: they hold no metric
        assert all(node < n0 for lst in got[1] for node in lst)
        assert not unpack_bits(np.array(got[2], np.uint64), n1)[:, n0:].any()
    plan, new_node = refresh_plan(c1, n0, 11)
    c2 = c1.reshaped(n1, m1, None)
    g2 = apply_refresh(ctx, gen + 1, c2, plan)
    check_get(ctx, g2, c2)
    got2 = answers(ctx, g2, n1, m1)
    if new_node is not None and plan:  # the new node stands at its place in the orders
        m = plan[0][1]
        rules = np.zeros(0, RULE_DTYPE)
        prio = np.array([(m, 0, 0), (m, 1, 0)], RULE_DTYPE)
        _, order, lens = ctx.tas_eval(g2, rules, np.zeros(3, np.int32), prio)
        assert order[0, 0] == new_node and order[1, lens[1] - 1] == new_node
    # the checker: the same content from scratch, then the same refresh
    c1.install(ctx, gen + 8)
    assert answers(ctx, gen + 8, n1, m1) == got
    g3 = apply_refresh(ctx, gen + 8, c1.reshaped(n1, m1, None), plan)
    assert answers(ctx, g3, n1, m1) == got2


@pytest.mark.gpu
def test_refusals_leave_the_snapshot(ctx):
    gen = next(_gen)
    c = make_content(3, 100, 3)
    c.install(ctx, gen)
    base = answers(ctx, gen, 100, 3)
    bad = [((gen + 1, gen + 2, 100, 3, None), _lib.PAS_ESTALE),
           ((gen, gen + 1, 99, 3, None), _lib.PAS_EINVAL),
           ((gen, gen + 1, 100, 3, [0, 1, 3]), _lib.PAS_EINVAL),
           ((gen, gen + 1, 100, 3, [0, -2, 1]), _lib.PAS_EINVAL),
           ((gen, gen + 1, 100, 3, [0, 0, 1]), _lib.PAS_EINVAL),
           ((gen, gen + 1, 100, 2, None), _lib.PAS_EINVAL),
           ((gen, gen + 1, 100, -1, None), _lib.PAS_EINVAL),
           # 3 * 2^20 * 2048 >= 2^31: arithmetic only, nothing of that size is allocated
           ((gen, gen + 1, 100, 1 << 20, None), _lib.PAS_ECAPACITY),
           ((gen, gen + 1, 100, 2**31 - 1, None), _lib.PAS_ECAPACITY),
           ((gen, gen + 1, (1 << 28), 3, None), _lib.PAS_ECAPACITY)]
    for args, code in bad:
        with pytest.raises(pas_amd.PasError) as e:
            ctx.tas_snapshot_reshape(*args)
        assert e.value.code == code, args
        ctx.n_nodes, ctx.n_metrics = 100, 3  # (the handle's shape follows successful calls only)
        assert ctx.tas_snapshot_info() == (gen, 100, 3)
    assert answers(ctx, gen, 100, 3) == base
    # the same shape with every column in place: only the generation moves
    ctx.tas_snapshot_reshape(gen, gen + 5, 100, 3, [0, 1, 2])
    ctx.tas_snapshot_reshape(gen + 5, gen + 6, 100, 3)
    assert ctx.tas_snapshot_info() == (gen + 6, 100, 3)
    assert answers(ctx, gen + 6, 100, 3) == base
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_eval(gen, *probe(3))
    assert e.value.code == _lib.PAS_ESTALE


@pytest.mark.gpu
def test_reshape_then_gas_topk(ctx):
    """Both snapshots grown to the same slots: the lazy top-k runs (no PAS_EINVAL for
    different node counts) and answers what freshly set snapshots answer."""
    import torch
    from pas_amd import workload as wl
    gen = next(_gen)
    n0, n1, P, k = 100, 130, 12, 6
    c0 = make_content(21, n0, 2)  # no wide column: the 64-bit records
    gs = wl.make_gas_snapshot(n0, seed=5)
    gb = wl.make_gas_batch(P, seed=5)
    rules, off, prio = probe(2)
    rules, off, prio = rules[:P], off[:P + 1], prio[:P]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def topk(tas_gen, gas_gen):
        key = torch.zeros((P, k), dtype=torch.int64, device="cuda")
        node = torch.zeros((P, k), dtype=torch.int32, device="cuda")
        ln = torch.zeros(P, dtype=torch.int32, device="cuda")
        ctx.tas_gas_topk_device(tas_gen, gas_gen, P, len(rules), dev(rules.view(np.uint8)),
                                dev(off), dev(prio.view(np.uint8)), None, gb.req.shape[1],
                                wl.I915, dev(gb.req), dev(gb.req_mask.view(np.int32)),
                                dev(gb.n_containers), k, 0, key, node, ln,
                                stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        ln = ln.cpu().numpy()
        return [[t.cpu().numpy()[p, :ln[p]].tolist() for p in range(P)] for t in (key, node)]

    c0.install(ctx, gen)
    ctx.gas_snapshot_set(gen + 1, gs.n_cards, gs.cap, gs.used)
    ctx.tas_snapshot_reshape(gen, gen + 2, n1, 2)
    ctx.gas_snapshot_resize(gen + 1, gen + 3, n1, gs.used.shape[1])
    got = topk(gen + 2, gen + 3)
    assert any(got[1])
    c0.reshaped(n1, 2, None).install(ctx, gen + 4)

    def grown(a, fill):
        return np.concatenate([a, np.full((n1 - n0,) + a.shape[1:], fill, a.dtype)])
    ctx.gas_snapshot_set(gen + 5, grown(gs.n_cards, -1), grown(gs.cap, 0), grown(gs.used, 0))
    assert topk(gen + 4, gen + 5) == got


# ------------------------------------------------------------------ no GPU

def test_header_and_library_declare_the_calls():
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in ("pas_tas_snapshot_reshape", "pas_tas_snapshot_get"):
        assert f"int {name}(" in header
        assert getattr(pas_amd.LIB, name).argtypes == _lib.SIGNATURES[name][1]
    assert "needs pas_tas_snapshot_set)" not in header
    for method in ("tas_snapshot_reshape", "tas_snapshot_get"):
        assert callable(getattr(pas_amd.Context, method))


def test_null_context_is_einval():
    assert pas_amd.LIB.pas_tas_snapshot_reshape(None, 0, 0, 0, 0, None, None) == _lib.PAS_EINVAL
    assert pas_amd.LIB.pas_tas_snapshot_get(None, None, None, None, None, None, None) == \
        _lib.PAS_EINVAL
