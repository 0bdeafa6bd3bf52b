"""Narrow (64-bit) metric columns at the int64 limits: the edge grid, the two snapshots built
from it, and the oracle pinned to the definition on them.  No GPU.

core.EvaluateRule (operator.go:13-26) and core.OrderedList (:30-42) on a narrow column at scale
s compare the value v * 10^-s with the integer target t exactly.  The definition below says
that in Python integers: v * 10^(9-s) against t * 10^9 with <, > and ==, the lists ascending or
descending with ties (and every other operator) in node order.  tests/test_narrow_limits.py
judges the kernels against the oracle's decimal form (or_*_dec, v_scale); nothing in
tests/golden/ reaches these values, so the oracle is first shown equal to the definition here.

The grid, for scale s (mult = 10^s, maxq = (2^63 - 1) // mult), clamped into int64:
  values   INT64_MIN + {0, 1, 2}, INT64_MAX - {0, 1, 2}, 0, +-1, +-mult, +-(mult - 1),
           +-(mult + 1), q * mult + d for q in {maxq, maxq - 1, -maxq, -maxq + 1}, d in -1..1
  targets  0, +-1, 2, INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, -INT64_MAX,
           +-maxq + d for d in -2..2
One snapshot holds all of it: column m at scale m for m in 0..9, column 10 with no node."""
import functools

import numpy as np
import pytest

from helpers import RULE_DTYPE, pack_bits, unpack_bits

I64_MIN, I64_MAX = -2**63, 2**63 - 1
LT, GT, EQ = 0, 1, 2
SCALES = list(range(10)) + [3]  # column 10: no node has it (milli, as a fresh column)
M = len(SCALES)
N_SMALL, N_LONG = 27, 2112


def _clamped(xs):
    out = []
    for x in xs:
        x = min(max(x, I64_MIN), I64_MAX)
        if x not in out:
            out.append(x)
    return out


def grid_values(s):
    mult = 10**s
    maxq = I64_MAX // mult
    xs = [I64_MIN, I64_MIN + 1, I64_MIN + 2, I64_MAX, I64_MAX - 1, I64_MAX - 2, 0, 1, -1,
          mult, -mult, mult - 1, -(mult - 1), mult + 1, -(mult + 1)]
    xs += [q * mult + d for q in (maxq, maxq - 1, -maxq, -maxq + 1) for d in (-1, 0, 1)]
    return _clamped(xs)


def grid_targets(s):
    maxq = I64_MAX // 10**s
    xs = [0, 1, -1, 2, I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - 1, -I64_MAX]
    xs += [sign * maxq + d for sign in (1, -1) for d in range(-2, 3)]
    return _clamped(xs)


# ------------------------------------------------------------------ the definition
def hit(v, s, op, t):
    """EvaluateRule on the value v * 10^-s and the integer target t."""
    a, b = int(v) * 10**(9 - s), int(t) * 10**9
    return a < b if op == LT else a > b if op == GT else a == b


class Definition:
    """Filter, sweep and ordered lists over v [M][N] (column m at scale SCALES[m]) and a
    presence matrix, in Python integers."""

    def __init__(self, v, pres_b, scales=SCALES):
        self.M, self.N = v.shape
        self.pres = np.asarray(pres_b, bool)
        self.scales = list(scales)
        self.big = [[int(x) * 10**(9 - scales[m]) for x in v[m].tolist()] for m in range(self.M)]

    def violating(self, rules):
        out = np.zeros(self.N, bool)
        for m, op, t in rules.tolist():
            if not 0 <= m < self.M:
                continue  # metric not cached: the rule is skipped
            b = t * 10**9
            col = self.big[m]
            if op == LT:
                h = [x < b for x in col]
            elif op == GT:
                h = [x > b for x in col]
            else:
                h = [x == b for x in col]
            out |= np.array(h, bool) & self.pres[m]
        return out

    def tas_violations(self, rules, off):
        return np.array([self.violating(rules[off[i]:off[i + 1]]) for i in range(len(off) - 1)],
                        bool).reshape(len(off) - 1, self.N)

    def tas_eval(self, rules, off, prio, cand_b=None):
        """(pass [P][N] bool, [list of node ids per pod])."""
        P = len(off) - 1
        ok = ~self.tas_violations(rules, off)
        if cand_b is not None:
            ok &= cand_b
        lists = []
        for p in range(P):
            m, op = int(prio[p]["metric"]), int(prio[p]["op"])
            if not 0 <= m < self.M:
                lists.append([])
                continue
            have = np.nonzero(ok[p] & self.pres[m])[0].tolist()
            col = self.big[m]
            if op == LT:
                have.sort(key=lambda n: col[n])  # stable: ties in node order
            elif op == GT:
                have.sort(key=lambda n: -col[n])
            lists.append(have)
        return ok, lists


# ------------------------------------------------------------------ the two snapshots
def _finish(v, pres_b):
    sc = np.repeat(np.array(SCALES, np.int8)[:, None], v.shape[1], 1)
    for a in (v, pres_b, sc):
        a.setflags(write=False)
    pres = pack_bits(pres_b)
    pres.setflags(write=False)
    return dict(v=v, pres_b=pres_b, pres=pres, sc=sc, N=v.shape[1])


@functools.lru_cache(maxsize=None)
def small_case():
    """N = 27: column m holds its 27 grid values (scale 0: its 12, then both limits again, then
    repeats), in a node order that is not the value order.  In each column one node that holds
    INT64_MAX and one that holds INT64_MIN are absent: their stored values must not leak, and
    at scale 0, where the limits stand on other nodes too, the absent nodes' sort keys tie with
    present limit values in both sorts.  (At the other scales the 27 values are distinct, so
    the present limits are the long snapshot's.)"""
    rng = np.random.default_rng(0x27)
    v = np.zeros((M, N_SMALL), np.int64)
    pres_b = np.ones((M, N_SMALL), bool)
    for s in range(10):
        vals = grid_values(s)
        col = (vals + [I64_MAX, I64_MIN] + vals * 2)[:N_SMALL]
        absent = [col.index(I64_MAX), col.index(I64_MIN)]
        order = rng.permutation(N_SMALL)
        v[s] = np.array(col, np.int64)[order]
        pres_b[s, np.nonzero(np.isin(order, absent))[0]] = False
    v[10] = rng.choice(np.array([I64_MIN, I64_MAX, 0, 1000], np.int64), N_SMALL)
    pres_b[10] = False
    return _finish(v, pres_b)


N_ABSENT = 3  # absent nodes per limit value and column of the long snapshot


@functools.lru_cache(maxsize=None)
def long_case():
    """N = 2112: every grid value of a column stands on more than 32 present nodes (a random
    33..60; the value 0, the middle of every column's grid, takes the rest), so every tie run
    of the ascending order is longer than a 32-block, and the run of 0 = 0 * mult lies over
    position 1024: a rule with target 0 has its bounds in different blocks of both fence
    levels.  Three more nodes per limit value hold it and are absent."""
    rng = np.random.default_rng(0x2112)
    v = np.zeros((M, N_LONG), np.int64)
    pres_b = np.ones((M, N_LONG), bool)
    n_present = N_LONG - 2 * N_ABSENT
    for s in range(10):
        vals = sorted(grid_values(s))
        reps = {x: int(rng.integers(33, 61)) for x in vals}
        reps[0] = n_present - sum(r for x, r in reps.items() if x != 0)
        col = [x for x in vals for _ in range(reps[x])]
        absent = [I64_MAX] * N_ABSENT + [I64_MIN] * N_ABSENT
        order = rng.permutation(N_LONG)
        v[s] = np.array(col + absent, np.int64)[order]
        pres_b[s] = order < n_present
    v[10] = rng.choice(np.array([I64_MIN, I64_MAX, 0, 1000], np.int64), N_LONG)
    pres_b[10] = False
    return _finish(v, pres_b)


CASES = {"small": small_case, "long": long_case}


def tie_runs(case, m):
    """[(value, start, end)] of the ascending order of column m's present values."""
    sv = np.sort(case["v"][m][case["pres_b"][m]])
    starts = np.nonzero(np.concatenate([[True], sv[1:] != sv[:-1]]))[0]
    ends = np.concatenate([starts[1:], [len(sv)]])
    return [(int(sv[a]), int(a), int(b)) for a, b in zip(starts, ends)]


def assert_long_shape(case):
    """The two conditions the long snapshot exists for, from its own arrays."""
    for s in range(10):
        runs = tie_runs(case, s)
        assert {x for x, _, _ in runs} == set(grid_values(s))
        assert min(b - a for _, a, b in runs) > 32, s
        products = {t * 10**s for t in grid_targets(s)}
        over = [(x, a, b) for x, a, b in runs if a < 1024 < b - 1 and x in products]
        assert over, s
        # both limits present, and absent nodes that hold them
        for lim in (I64_MIN, I64_MAX):
            assert (case["v"][s][~case["pres_b"][s]] == lim).sum() == N_ABSENT
            assert (case["v"][s][case["pres_b"][s]] == lim).sum() > 32
    assert not case["pres_b"][10].any()


# ------------------------------------------------------------------ rules
@functools.lru_cache(maxsize=None)
def single_rules():
    """One single-rule pod (strategy, policy) per (metric, operator, target) of the grid, the
    prioritize operators cycling 0..3 over the rule's own metric."""
    rules = np.array([(m, op, t) for m in range(10) for op in range(3) for t in grid_targets(m)],
                     RULE_DTYPE)
    off = np.arange(len(rules) + 1, dtype=np.int32)
    prio = np.array([(r["metric"], p % 4, 0) for p, r in enumerate(rules)], RULE_DTYPE)
    for a in (rules, off, prio):
        a.setflags(write=False)
    return rules, off, prio


def mixed_batch(n, seed=0x48, pods=48, per_pod=3, cand_frac=0.85):
    """Pods of several rules over all 11 columns, each target from its column's grid, any
    prioritize metric and operator 0..3, and a candidate mask."""
    rng = np.random.default_rng(seed)
    rules = []
    for _ in range(pods * per_pod):
        m = int(rng.integers(0, M))
        ts = grid_targets(SCALES[m])
        rules.append((m, int(rng.integers(0, 3)), ts[int(rng.integers(0, len(ts)))]))
    off = np.arange(0, len(rules) + 1, per_pod, dtype=np.int32)
    prio = np.array([(int(rng.integers(0, M)), int(rng.integers(0, 4)), 0) for _ in range(pods)],
                    RULE_DTYPE)
    cand_b = rng.random((pods, n)) < cand_frac
    return np.array(rules, RULE_DTYPE), off, prio, cand_b


def limit_strategies():
    """64 single-rule strategies (the label plan's limit): every operator against both int64
    limits on every column, and four rules on the targets next to them."""
    rules = [(m, op, t) for m in range(10) for t in (I64_MIN, I64_MAX) for op in range(3)]
    rules += [(0, GT, I64_MIN + 1), (0, LT, I64_MAX - 1), (9, EQ, 0), (5, GT, -1)]
    assert len(rules) == 64
    return np.array(rules, RULE_DTYPE), np.arange(65, dtype=np.int32)


# ------------------------------------------------------------------ CPU tests
def test_grid_sizes():
    assert len(grid_values(0)) == 12 and len(grid_targets(0)) == 11
    for s in range(1, 10):
        assert len(grid_values(s)) == 27 and len(grid_targets(s)) == 18, s
    rules, _, _ = single_rules()
    per_metric = np.bincount(rules["metric"], minlength=10).tolist()
    assert per_metric == [33] + [54] * 9


def test_oracle_equals_definition_on_every_triple(oracle):
    """Every (value, operator, target) of the grid through oracle.tas_violations, a strategy
    per rule over the column of the scale's values."""
    triples = 0
    for s in range(10):
        vals, ts = grid_values(s), grid_targets(s)
        v = np.array([vals], np.int64)
        pres = pack_bits(np.ones((1, len(vals)), bool))
        rules = np.array([(0, op, t) for op in range(3) for t in ts], RULE_DTYPE)
        off = np.arange(len(rules) + 1, dtype=np.int32)
        got = unpack_bits(oracle.tas_violations(v, pres, rules, off,
                                                v_scale=np.full((1, len(vals)), s, np.int8)),
                          len(vals))
        for i, (_, op, t) in enumerate(rules.tolist()):
            for j, x in enumerate(vals):
                assert bool(got[i, j]) == hit(x, s, op, t), (s, x, op, t)
                triples += 1
    assert triples == 13_518
    # the two triples the saturating restatement of the kernels got wrong
    assert not hit(I64_MIN, 0, GT, I64_MIN) and hit(I64_MIN, 0, EQ, I64_MIN)


def test_long_snapshot_holds_what_it_claims():
    assert_long_shape(long_case())
    small = small_case()
    for s in range(10):
        gone = small["v"][s][~small["pres_b"][s]].tolist()
        assert sorted(gone) == [I64_MIN, I64_MAX], s
    there = small["v"][0][small["pres_b"][0]].tolist()
    assert I64_MIN in there and I64_MAX in there


@pytest.mark.parametrize("kind", ["small", "long"])
def test_oracle_lists_equal_definition(oracle, kind):
    """Pass rows and ordered lists of the single-rule pods (prioritize operators 0, 1, 2 and 3)
    and of the mixed batch with candidates, on both snapshots."""
    case = CASES[kind]()
    n = case["N"]
    d = Definition(case["v"], case["pres_b"])
    r2, o2, p2, c2 = mixed_batch(n)
    assert set(single_rules()[2]["op"].tolist()) == {0, 1, 2, 3}
    for rules, off, prio, cand_b in (single_rules() + (None,), (r2, o2, p2, c2)):
        cand = None if cand_b is None else pack_bits(cand_b)
        gp, go, gl = oracle.tas_eval(case["v"], case["pres"], rules, off, prio, cand,
                                     v_scale=case["sc"])
        ok, lists = d.tas_eval(rules, off, prio, cand_b)
        np.testing.assert_array_equal(unpack_bits(gp, n), ok)
        assert gl.tolist() == [len(x) for x in lists]
        for p, want in enumerate(lists):
            assert go[p, :gl[p]].tolist() == want, f"pod {p}"
        np.testing.assert_array_equal(
            unpack_bits(oracle.tas_violations(case["v"], case["pres"], rules, off,
                                              v_scale=case["sc"]), n),
            d.tas_violations(rules, off))
