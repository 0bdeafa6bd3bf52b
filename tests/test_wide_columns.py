"""Wide metric columns: values that do not fit int64 at one decimal scale, as (whole, nano)
pairs (include/pas.h, pas_tas_snapshot_update_wide; DESIGN.md "Wide columns").

The reference compares every resource.Quantity exactly: EvaluateRule with CmpInt64 and
OrderedList with Cmp (telemetry-aware-scheduling/pkg/strategies/core/operator.go:13-42).
Two checkers:
  * the oracle's per-value decimal form (oracle.tas_eval(..., v_scale=s), tas_violations,
    prioritize_request), for every value that is int64 u * 10^-s;
  * `Restated`, a short restatement of operator.go:13-42 on exact Decimals (go_value, at
    precision 80) with the tie rules of pas.h, for values outside that form.  It is first
    shown equal to the oracle on every oracle-representable case used here (CPU test), and
    only then used as a checker.
"""
import json
from decimal import Decimal

import numpy as np
import pytest

import pas_amd
from pas_amd import snapshot as sn
from pas_amd.workload import pack_bits
from helpers import RULE_DTYPE, unpack_bits
from test_quantity_scaled import CASES, go_value, want_decimals

I64_MAX, I64_MIN = 2**63 - 1, -2**63
ENOTEXACT = pas_amd._lib.PAS_ENOTEXACT
EINVAL = pas_amd._lib.PAS_EINVAL
ESTALE = pas_amd._lib.PAS_ESTALE

COUNTER = ["1e16", "12345678901234567", "9223372036854775807", "-9223372036854775807",
           "9223372036854775806", "0", "1", "1e16", "-1e16", "9e15",
           "12345678901234567", "9223372036854775807", "2", "3", "10000000000000001",
           "9999999999999999", "-1", "1e16", "0", "1000000000000", "-9223372036854775807",
           "12345678901234568", "9e15", "1e12"]
MIXED = ["1e-7", "1e12", "99999999999.9999999", "-1e-7", "0.5", "-0.5", "1e12",
         "1000000000000.000001", "-1e12", "2.000000001", "-2.000000001", "2", "3", "-3",
         "1e-7", "0.5", "2", "0", "1", "-1", "2.000000001", "1000000000000", "-1n", "1e12"]
TEMP = ["70", "71", "69", "70", "72", "68", "70", "75", "60", "80", "70", "71", "69", "70",
        "72", "68", "1.5", "2", "3", "-3", "0", "1", "2", "70"]
# past the oracle's form (no int64 u at the value's own decimal places), and integers next
# to them
PAST = ["9000000000000000000.5", "9000000000000000000.25", "-9000000000000000000.5",
        "4611686018427387904.000000001", "1000000000000.0000001",
        "9223372036854775806.999999999", "9000000000000000000", "9000000000000000001",
        "-9000000000000000001", "-9000000000000000000", "4611686018427387904",
        "4611686018427387905", "1000000000000", "1000000000001", "9223372036854775806",
        "9223372036854775807", "9000000000000000000.5", "0", "-0.5", "1",
        "9000000000000000000.25", "1000000000000.0000001", "-9223372036854775807", "2"]
TARGETS = [-3, -2, -1, 0, 1, 2, 3, 10**12, 10**16, I64_MAX, -I64_MAX, I64_MIN]
PAST_TARGETS = TARGETS + [9 * 10**18, 9 * 10**18 + 1, -9 * 10**18, -9 * 10**18 - 1, 2**62,
                          2**62 + 1, 10**12 + 1, I64_MAX - 1]


def wide_pair(v: Decimal):
    """(whole, nano) of an exact value with at most 9 decimal places: whole the floor."""
    n = int(v.scaleb(9))
    assert Decimal(n).scaleb(-9) == v
    return n // 10**9, n % 10**9  # Python's // floors


def exact_decimal(lit):
    v = go_value(lit)
    s = want_decimals(v)
    return int(v.scaleb(s)), s


def bit(words, i):
    return (int(words[i >> 6]) >> (i & 63)) & 1


# ------------------------------------------------------------------ the restatement
class Restated:
    """operator.go:13-42 over vals[m][n] (Decimal, or None where the node has no metric).
    EvaluateRule: LessThan value < target, GreaterThan value > target, Equals value ==
    target (CmpInt64 is exact).  OrderedList: GreaterThan descending, LessThan ascending, any
    other operator unsorted; ties and the unsorted case in ascending node index (batched
    eval) or ascending request position (one request), as pas.h fixes them."""

    def __init__(self, vals):
        self.vals = vals
        self.M, self.N = len(vals), len(vals[0])

    @staticmethod
    def hit(v, op, t):
        return v < t if op == 0 else v > t if op == 1 else v == t

    def _violating(self, rules):
        out = np.zeros(self.N, bool)
        for m, op, t in rules:
            if not 0 <= m < self.M:
                continue  # metric not cached: the rule is skipped
            for n, v in enumerate(self.vals[m]):
                if v is not None and self.hit(v, int(op), int(t)):
                    out[n] = True
        return out

    def tas_violations(self, rules, off):
        rows = [self._violating(rules[off[s]:off[s + 1]]) for s in range(len(off) - 1)]
        return pack_bits(np.array(rows).reshape(len(off) - 1, self.N))

    def tas_eval(self, rules, off, prio, cand=None):
        P = len(off) - 1
        passed = np.zeros((P, self.N), bool)
        order = np.zeros((P, self.N), np.int32)
        lens = np.zeros(P, np.int32)
        for p in range(P):
            c = unpack_bits(cand[p:p + 1], self.N)[0] if cand is not None else \
                np.ones(self.N, bool)
            passed[p] = c & ~self._violating(rules[off[p]:off[p + 1]])
            m, op = int(prio[p]["metric"]), int(prio[p]["op"])
            if not 0 <= m < self.M:
                continue
            have = [n for n in range(self.N) if passed[p, n] and self.vals[m][n] is not None]
            if op == 0:
                have.sort(key=lambda n: self.vals[m][n])  # stable: ties in node order
            elif op == 1:
                have.sort(key=lambda n: -self.vals[m][n])
            lens[p] = len(have)
            order[p, :len(have)] = have
        return pack_bits(passed), order, lens

    def prioritize_request(self, prio, req):
        m, op = int(prio["metric"]), int(prio["op"])
        if not 0 <= m < self.M:
            return np.zeros(0, np.int32)
        seen, pos = set(), []
        for j, n in enumerate(req):
            if 0 <= n < self.N and n not in seen:
                seen.add(int(n))
                if self.vals[m][n] is not None:
                    pos.append(j)
        if op == 0:
            pos.sort(key=lambda j: self.vals[m][req[j]])
        elif op == 1:
            pos.sort(key=lambda j: -self.vals[m][req[j]])
        return np.array(pos, np.int32)


class OracleChecker:
    """The oracle's per-value decimal form behind Restated's interface."""

    def __init__(self, oracle, u, s, pres):
        self.o, self.u, self.s, self.pres = oracle, u, s, pres

    def tas_violations(self, rules, off):
        return self.o.tas_violations(self.u, self.pres, rules, off, v_scale=self.s)

    def tas_eval(self, rules, off, prio, cand=None):
        return self.o.tas_eval(self.u, self.pres, rules, off, prio, cand, v_scale=self.s)

    def prioritize_request(self, prio, req):
        return self.o.prioritize_request(self.u, self.pres, prio, req, v_scale=self.s)


# ------------------------------------------------------------------ cases
def literal_columns(cols, absent=()):
    """nodes, metrics {name: {node: literal}}, names for columns of literals; absent =
    {(name, node index)} left out."""
    n = len(next(iter(cols.values())))
    nodes = [f"node-{i}" for i in range(n)]
    metrics = {name: {nodes[i]: lit for i, lit in enumerate(col) if (name, i) not in absent}
               for name, col in cols.items()}
    return nodes, metrics, list(cols)


def decimal_matrix(metrics, nodes, names):
    return [[go_value(metrics[name][n]) if n in metrics[name] else None for n in nodes]
            for name in names]


def oracle_arrays(metrics, nodes, names):
    """Per-value (u, s) with |u| < 2^63 at the value's own decimal places, and presence."""
    M, N = len(names), len(nodes)
    u = np.zeros((M, N), np.int64)
    s = np.zeros((M, N), np.int8)
    pres = np.zeros((M, N), bool)
    for m, name in enumerate(names):
        for i, node in enumerate(nodes):
            if node in metrics[name]:
                uu, ss = exact_decimal(metrics[name][node])
                assert I64_MIN <= uu <= I64_MAX, (name, metrics[name][node])
                u[m, i], s[m, i], pres[m, i] = uu, ss, True
    return u, s, pack_bits(pres)


def rule_batch(rng, M, P, R, targets):
    rules, off = [], [0]
    prio = np.zeros(P, RULE_DTYPE)
    for p in range(P):
        for _ in range(R):
            rules.append((int(rng.integers(0, M)), int(rng.integers(0, 3)),
                          int(targets[int(rng.integers(0, len(targets)))])))
        off.append(len(rules))
        prio[p] = (int(rng.integers(0, M)), int(rng.integers(0, 3)), 0)
    return np.array(rules, RULE_DTYPE), np.array(off, np.int32), prio


def every_rule(M, targets):
    """One single-rule pod (or strategy) per (metric, operator, target)."""
    rules = np.array([(m, op, t) for m in range(M) for op in range(3) for t in targets],
                     RULE_DTYPE)
    return rules, np.arange(len(rules) + 1, dtype=np.int32)


LITERAL = literal_columns({"counter": COUNTER, "mixed": MIXED, "temp": TEMP},
                          absent={("mixed", 7)})
PAST_CASE = literal_columns({"past": PAST, "temp": TEMP}, absent={("past", 17)})


def requests_for(rng, n):
    """Request node lists with repeated and unknown (-1, past the end) nodes."""
    a = rng.permutation(n).astype(np.int32)
    b = rng.integers(-1, n + 2, 3 * n).astype(np.int32)
    b[b >= n] = -1
    return [a, b, np.concatenate([a[: n // 2], a[: n // 2], [-1]]).astype(np.int32)]


# ------------------------------------------------------------------ CPU tests
def test_quantity_to_wide_literals():
    lits = CASES + COUNTER + MIXED + PAST + ["-0.5", "-1n", "0"]
    for lit in lits:
        assert pas_amd.quantity_to_wide(lit) == wide_pair(go_value(lit)), lit
    assert pas_amd.quantity_to_wide("-0.5") == (-1, 500000000)
    assert pas_amd.quantity_to_wide("-1n") == (-1, 999999999)
    assert pas_amd.quantity_to_wide("1e16") == (10**16, 0)


def test_quantity_to_wide_random_literals():
    rng = np.random.default_rng(0x71DE)
    for _ in range(3000):
        frac = int(rng.integers(0, 12))
        ip = int(rng.integers(0, 10**int(rng.integers(0, 19))))
        fp = int(rng.integers(0, 10**min(frac, 18))) if frac else 0
        sign = "-" if rng.random() < 0.3 else ""
        body = f"{sign}{ip}" + (f".{fp:0{frac}d}" if frac else "")
        suf = ["", "", "m", "u", "n", "k", "M", f"e-{int(rng.integers(1, 4))}",
               f"e{int(rng.integers(1, 4))}"][int(rng.integers(0, 9))]
        lit = body + suf
        v = go_value(lit)
        whole = int(v.scaleb(9)) // 10**9
        if I64_MIN <= whole <= I64_MAX:
            assert pas_amd.quantity_to_wide(lit) == wide_pair(v), lit
        else:
            with pytest.raises(pas_amd.PasError) as e:
                pas_amd.quantity_to_wide(lit)
            assert e.value.code == ENOTEXACT, lit


def test_quantity_to_wide_errors():
    for lit in ("1e19", "-1e19"):
        with pytest.raises(pas_amd.PasError) as e:
            pas_amd.quantity_to_wide(lit)
        assert e.value.code == ENOTEXACT
    with pytest.raises(pas_amd.PasError) as e:
        pas_amd.quantity_to_wide("1.2.3")
    assert e.value.code == EINVAL


def test_builder_wide_keeps_narrow_columns():
    metrics = {"m1": {"a": "1.5", "b": "2", "zz": "7"}, "m2": {"b": "1m", "a": "0.0001"},
               "m4": {"a": "1e-7", "b": "1500u"}, "m5": {"a": "9e15"}}
    names = ["m1", "m2", "m3", "m4", "m5"]
    v0, p0, s0 = sn.tas_snapshot_from_metrics(metrics, ["a", "b"], names)
    v, p, s, wide = sn.tas_snapshot_from_metrics_wide(metrics, ["a", "b"], names)
    np.testing.assert_array_equal(v, v0)
    np.testing.assert_array_equal(p, p0)
    np.testing.assert_array_equal(s, s0)
    assert v.dtype == v0.dtype and p.dtype == p0.dtype and s.dtype == s0.dtype
    assert wide == {}


def test_builder_wide_columns():
    v, p, s, wide = sn.tas_snapshot_from_metrics_wide(
        {"big": {"a": "1e-7", "b": "1e12"}, "ok": {"a": "1"}}, ["a", "b"])
    assert list(wide) == [0] and v[0].tolist() == [0, 0] and int(p[0, 0]) == 0b11
    assert wide[0][0].tolist() == [0, 10**12] and wide[0][1].tolist() == [100, 0]
    assert wide[0][0].dtype == np.int64 and wide[0][1].dtype == np.uint32
    assert v[1].tolist() == [1000, 0] and int(p[1, 0]) == 0b01
    v, p, s, wide = sn.tas_snapshot_from_metrics_wide({"m": {"a": "1e16"}}, ["a", "b"])
    assert wide[0][0].tolist() == [10**16, 0] and wide[0][1].tolist() == [0, 0]
    assert int(p[0, 0]) == 0b01
    with pytest.raises(pas_amd.PasError) as e:
        sn.tas_snapshot_from_metrics_wide({"huge": {"a": "1e19", "b": "1e-7"}}, ["a", "b"])
    assert e.value.code == ENOTEXACT and "huge" in str(e.value)


def test_restatement_equals_oracle(oracle):
    """The Decimal restatement against the oracle on every oracle-representable case of the
    GPU tests below: the literal snapshot with every (metric, operator, target) rule, random
    rule batches with candidates, the sweep, and the request prioritize."""
    nodes, metrics, names = LITERAL
    u, s, pres = oracle_arrays(metrics, nodes, names)
    chk, rs = OracleChecker(oracle, u, s, pres), Restated(decimal_matrix(metrics, nodes, names))
    rng = np.random.default_rng(0xE0)
    N, M = len(nodes), len(names)
    rules, off = every_rule(M, TARGETS)
    np.testing.assert_array_equal(rs.tas_violations(rules, off), chk.tas_violations(rules, off))
    for batch in ((rules, off, rule_batch(rng, M, len(rules), 0, TARGETS)[2], None),
                  rule_batch(rng, M, 64, 3, TARGETS) + (pack_bits(rng.random((64, N)) < 0.8),)):
        a, b = rs.tas_eval(*batch), chk.tas_eval(*batch)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[2], b[2])
        for p in range(len(a[2])):
            np.testing.assert_array_equal(a[1][p, :a[2][p]], b[1][p, :b[2][p]])
    for m in range(M):
        for op in range(3):
            pr = np.array([(m, op, 0)], RULE_DTYPE)[0]
            for req in requests_for(rng, N):
                np.testing.assert_array_equal(rs.prioritize_request(pr, req),
                                              chk.prioritize_request(pr, req))


# ------------------------------------------------------------------ GPU tests
def check_paths(ctx, gen, chk, N, M, rng, targets, n_strat=6):
    """Filter + prioritize, the sweep, the fused deschedule with its label plan, and request
    prioritize with repeated and unknown nodes: every word and every list entry."""
    from pas_amd import workload as wl
    from test_labels import _fused_and_separate
    rules, off = every_rule(M, targets)
    prio = rule_batch(rng, M, len(rules), 0, targets)[2]
    r2, o2, p2 = rule_batch(rng, M, 48, 3, targets)
    cand = pack_bits(rng.random((48, N)) < 0.85)
    for batch in ((rules, off, prio, None), (r2, o2, p2, cand)):
        gp, go, gl = ctx.tas_eval(gen, *batch)
        wp, wo, wlens = chk.tas_eval(*batch)
        np.testing.assert_array_equal(gp, wp)
        np.testing.assert_array_equal(gl, wlens)
        for p in range(len(gl)):
            np.testing.assert_array_equal(go[p, :gl[p]], wo[p, :wlens[p]], err_msg=f"pod {p}")
    # the sweep over every single rule (two-call form), then strategies of several rules
    np.testing.assert_array_equal(ctx.tas_violations(gen, rules, off),
                                  chk.tas_violations(rules, off))
    dr, doff, _ = rule_batch(rng, M, n_strat, 2, targets)
    want_v = chk.tas_violations(dr, doff)
    labels = wl.pack_bits(rng.random((n_strat, N)) < 0.5)
    f, sep = _fused_and_separate(ctx, gen, N, n_strat, dr, doff, labels)
    np.testing.assert_array_equal(f[0], want_v)
    np.testing.assert_array_equal(sep[0], want_v)
    import oracle as orc
    want = orc.label_plan(want_v, labels, N)
    for i in (1, 2):
        np.testing.assert_array_equal(f[i], want[i - 1])
        np.testing.assert_array_equal(sep[i], want[i - 1])
    assert f[3] == sep[3] == want[2]
    for m in range(M):
        for op in range(3):
            pr = np.array([(m, op, 0)], RULE_DTYPE)[0]
            for req in requests_for(rng, N):
                np.testing.assert_array_equal(ctx.tas_prioritize_request(gen, pr, req),
                                              chk.prioritize_request(pr, req),
                                              err_msg=f"metric {m} op {op}")


@pytest.mark.gpu
def test_literal_snapshot_all_paths(ctx, oracle):
    nodes, metrics, names = LITERAL
    v, pres, scale, wide = sn.tas_snapshot_from_metrics_wide(metrics, nodes, names)
    assert sorted(wide) == [0, 1]
    u, s, opres = oracle_arrays(metrics, nodes, names)
    np.testing.assert_array_equal(pres, opres)
    ctx.tas_snapshot_set_wide(9500, v, pres, scale, wide)
    assert ctx.tas_snapshot_wide_count() == 2
    assert ctx.tas_snapshot_info()[0] == 9500
    check_paths(ctx, 9500, OracleChecker(oracle, u, s, opres), len(nodes), len(names),
                np.random.default_rng(0x11), TARGETS)


@pytest.mark.gpu
def test_verdict_list(ctx, oracle):
    """1e16, 12345678901234567, +-(2^63 - 1), and 1e-7 mixed with 1e12, from Quantity strings
    through the wide builder, on every path."""
    cols = {"bytes": ["1e16", "12345678901234567", "9223372036854775807",
                      "-9223372036854775807", "1e16", "0"],
            "ratio": ["1e-7", "1e12", "1e-7", "1e12", "0", "1"]}
    nodes, metrics, names = literal_columns(cols)
    v, pres, scale, wide = sn.tas_snapshot_from_metrics_wide(metrics, nodes, names)
    assert sorted(wide) == [0, 1]
    u, s, opres = oracle_arrays(metrics, nodes, names)
    ctx.tas_snapshot_set_wide(9510, v, pres, scale, wide)
    check_paths(ctx, 9510, OracleChecker(oracle, u, s, opres), len(nodes), len(names),
                np.random.default_rng(0x12), TARGETS, n_strat=4)


@pytest.mark.gpu
def test_past_the_oracle_form(ctx):
    nodes, metrics, names = PAST_CASE
    v, pres, scale, wide = sn.tas_snapshot_from_metrics_wide(metrics, nodes, names)
    assert sorted(wide) == [0]
    ctx.tas_snapshot_set_wide(9520, v, pres, scale, wide)
    check_paths(ctx, 9520, Restated(decimal_matrix(metrics, nodes, names)), len(nodes),
                len(names), np.random.default_rng(0x13), PAST_TARGETS)


def random_wide(rng, N):
    """(whole, nano) drawn from two oracle-representable classes in one column, with heavy
    ties: any int64 whole but -2^63 with nano 0; |whole| < 1e9 with any nano."""
    whole = np.zeros(N, np.int64)
    nano = np.zeros(N, np.uint32)
    big = rng.random(N) < 0.5
    pool = np.concatenate([rng.integers(-I64_MAX, I64_MAX, 40, dtype=np.int64, endpoint=True),
                           np.array([I64_MAX, -I64_MAX, I64_MAX - 1, 0, 1, -1], np.int64)])
    whole[big] = rng.choice(pool, int(big.sum()))
    small_w = rng.integers(-5, 6, 30)  # equal wholes, different nanos
    small_n = np.concatenate([rng.integers(0, 10**9, 12), [0, 0, 1, 999_999_999, 500_000_000]])
    k = int((~big).sum())
    whole[~big] = rng.choice(small_w, k)
    nano[~big] = rng.choice(small_n, k)
    far = ~big & (rng.random(N) < 0.2)
    whole[far] = rng.integers(-10**9 + 1, 10**9, int(far.sum()))
    return whole, nano


def wide_oracle_values(whole, nano):
    """(u, s) of the two classes: (whole, 0) and (whole * 1e9 + nano, 9)."""
    frac = nano != 0
    small = np.abs(whole) < 10**9
    assert np.all(~frac | small)
    u = np.where(frac, whole * 10**9 + nano.astype(np.int64), whole)
    return u, np.where(frac, 9, 0).astype(np.int8)


@pytest.mark.gpu
def test_random_wide_direct_api(ctx, oracle):
    from pas_amd import workload as wl
    from test_labels import _fused_and_separate
    rng = np.random.default_rng(0x2100)
    N, M, wide_cols = 2100, 6, [1, 3, 4]
    v = rng.integers(-10**6, 10**6, (M, N)).astype(np.int64)  # narrow: milli
    pres_b = rng.random((M, N)) < 0.9
    pres = pack_bits(pres_b)
    u, s = v.copy(), np.full((M, N), 3, np.int8)
    whole = np.zeros((len(wide_cols), N), np.int64)
    nano = np.zeros((len(wide_cols), N), np.uint32)
    for c, m in enumerate(wide_cols):
        whole[c], nano[c] = random_wide(rng, N)
        u[m], s[m] = wide_oracle_values(whole[c], nano[c])
    gen = 9530
    ctx.tas_snapshot_set(gen, v, pres)
    ctx.tas_snapshot_update_wide(gen, gen + 1, wide_cols, whole, nano, pres[wide_cols])
    gen += 1
    assert ctx.tas_snapshot_wide_count() == 3
    seen = np.unique(whole[:, ::7])  # the wholes present +- 1, and the int64 limits
    targets = sorted({min(max(int(w) + d, I64_MIN), I64_MAX) for w in seen for d in (-1, 0, 1)}
                     | {I64_MAX, I64_MIN, -I64_MAX, 0})
    chk = OracleChecker(oracle, u, s, pres)
    rules, off, prio = rule_batch(rng, M, 64, 3, targets)
    cand = pack_bits(rng.random((64, N)) < 0.9)
    gp, go, gl = ctx.tas_eval(gen, rules, off, prio, cand)
    wp, wo, wlens = chk.tas_eval(rules, off, prio, cand)
    np.testing.assert_array_equal(gp, wp)
    np.testing.assert_array_equal(gl, wlens)
    for p in range(64):
        np.testing.assert_array_equal(go[p, :gl[p]], wo[p, :wlens[p]], err_msg=f"pod {p}")
    # prioritize alone over every wide order
    pr = np.array([(m, op, 0) for m in wide_cols for op in range(3)], RULE_DTYPE)
    none = (np.zeros(0, RULE_DTYPE), np.zeros(len(pr) + 1, np.int32))
    _, go, gl = ctx.tas_eval(gen, *none, pr)
    _, wo, wlens = chk.tas_eval(*none, pr)
    np.testing.assert_array_equal(gl, wlens)
    for p in range(len(pr)):
        np.testing.assert_array_equal(go[p, :gl[p]], wo[p, :wlens[p]], err_msg=f"order {p}")
    dr, doff, _ = rule_batch(rng, M, 8, 3, targets)
    want_v = chk.tas_violations(dr, doff)
    labels = wl.pack_bits(rng.random((8, N)) < 0.3)
    f, sep = _fused_and_separate(ctx, gen, N, 8, dr, doff, labels)
    np.testing.assert_array_equal(f[0], want_v)
    np.testing.assert_array_equal(sep[0], want_v)
    want = oracle.label_plan(want_v, labels, N)
    for i in (1, 2):
        np.testing.assert_array_equal(f[i], want[i - 1])
        np.testing.assert_array_equal(sep[i], want[i - 1])
    assert f[3] == sep[3] == want[2]
    for m in wide_cols + [0]:
        for op in range(3):
            one = np.array([(m, op, 0)], RULE_DTYPE)[0]
            for req in requests_for(rng, N)[:2]:
                np.testing.assert_array_equal(ctx.tas_prioritize_request(gen, one, req),
                                              chk.prioritize_request(one, req))


@pytest.mark.gpu
def test_long_row_chunked_fences(ctx, oracle):
    """140 000 nodes: more than 128 fences of 1024, the chunked fence loop of the range
    search."""
    rng = np.random.default_rng(0x140)
    N = 140_000
    whole, nano = random_wide(rng, N)
    # mostly distinct values, so that the bounds fall in every part of the row
    spread = rng.random(N) < 0.8
    whole[spread] = rng.integers(-10**8, 10**8, int(spread.sum()))
    nano[spread] = rng.integers(0, 10**9, int(spread.sum()))
    pres = pack_bits((rng.random((1, N)) < 0.97))
    u, s = wide_oracle_values(whole, nano)
    ctx.tas_snapshot_set(9540, np.zeros((1, N), np.int64), pres)
    ctx.tas_snapshot_update_wide(9540, 9541, [0], whole[None], nano[None], pres)
    t = np.sort(whole[spread])[[10, 40_000, 70_000, 100_000]]
    rules = np.array([(0, 0, t[0]), (0, 2, 0), (0, 1, t[3]), (0, 2, t[1]), (0, 0, -10**8),
                      (0, 1, t[2] + 10**7 * 9), (0, 1, I64_MAX - 1), (0, 0, -I64_MAX)],
                     RULE_DTYPE)
    off = np.array([0, 2, 4, 6, 8], np.int32)
    prio = np.array([(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 1, 0)], RULE_DTYPE)
    gp, go, gl = ctx.tas_eval(9541, rules, off, prio)
    wp, wo, wlens = oracle.tas_eval(u[None], pres, rules, off, prio, v_scale=s[None])
    np.testing.assert_array_equal(gp, wp)
    np.testing.assert_array_equal(gl, wlens)
    for p in range(4):
        np.testing.assert_array_equal(go[p, :gl[p]], wo[p, :wlens[p]], err_msg=f"pod {p}")


@pytest.mark.gpu
def test_bounds_in_different_fence_blocks(ctx, oracle):
    """2100 present nodes (two 1024-blocks, a last 32-block of 20) whose sorted row holds a run
    of equal pairs over position 1024: the 1024-fence equals the target, so the lower and the
    upper bound of a rule on it are searched in different blocks of both fence levels."""
    rng = np.random.default_rng(0x1024)
    N = 2100
    i = np.arange(N)
    whole = np.where(i < 1000, i - 3000, np.where(i <= 1100, 7, 8 + (i - 1101) // 2))
    nano = np.where(i < 1000, 5, np.where(i <= 1100, 0, (i - 1101) % 2 * 500_000_000))
    order = rng.permutation(N)  # node order is not value order
    whole, nano = whole[order].astype(np.int64), nano[order].astype(np.uint32)
    pres = pack_bits(np.ones((1, N), bool))
    u, s = wide_oracle_values(whole, nano)
    ctx.tas_snapshot_set(9545, np.zeros((1, N), np.int64), pres)
    ctx.tas_snapshot_update_wide(9545, 9546, [0], whole[None], nano[None], pres)
    last = int(whole.max())
    targets = [7, 6, 8, -2001, -2000, last, last + 1, -3001]
    rules = np.array([(0, op, t) for t in targets for op in range(3)], RULE_DTYPE)
    off = np.arange(len(rules) + 1, dtype=np.int32)  # one rule per pod
    prio = np.array([(0, p % 3, 0) for p in range(len(rules))], RULE_DTYPE)
    gp, go, gl = ctx.tas_eval(9546, rules, off, prio)
    wp, wo, wlens = oracle.tas_eval(u[None], pres, rules, off, prio, v_scale=s[None])
    np.testing.assert_array_equal(gp, wp)
    np.testing.assert_array_equal(gl, wlens)
    for p in range(len(rules)):
        np.testing.assert_array_equal(go[p, :gl[p]], wo[p, :wlens[p]], err_msg=f"pod {p}")
    # by hand for target 7: 1000 nodes below it, 999 above it, the run of 101 equal to it
    failed = [N - sum(int(w).bit_count() for w in gp[p]) for p in range(3)]
    assert failed == [1000, 999, 101]


@pytest.mark.gpu
def test_transitions_and_errors(ctx, oracle):
    import torch
    rng = np.random.default_rng(0x7A)
    N, M = 300, 3
    v = rng.integers(-5000, 5000, (M, N)).astype(np.int64)
    pres = pack_bits(rng.random((M, N)) < 0.9)
    scale = [3, 4, 0]
    targets = [-2, -1, 0, 1, 2, 10**12]
    rules, off, prio = rule_batch(rng, M, 32, 2, targets)
    dr, doff, _ = rule_batch(rng, M, 4, 2, targets)

    def check(gen, u, s):
        gp, go, gl = ctx.tas_eval(gen, rules, off, prio)
        wp, wo, wlens = oracle.tas_eval(u, pres, rules, off, prio, v_scale=s)
        np.testing.assert_array_equal(gp, wp)
        np.testing.assert_array_equal(gl, wlens)
        for p in range(len(gl)):
            np.testing.assert_array_equal(go[p, :gl[p]], wo[p, :wlens[p]])
        np.testing.assert_array_equal(ctx.tas_violations(gen, dr, doff),
                                      oracle.tas_violations(u, pres, dr, doff, v_scale=s))

    s0 = np.repeat(np.array(scale, np.int8)[:, None], N, 1)
    ctx.tas_snapshot_set(9550, v, pres, scale)
    assert ctx.tas_snapshot_wide_count() == 0
    check(9550, v, s0)
    # narrow -> wide on column 1
    whole, nano = random_wide(rng, N)
    u1, s1 = v.copy(), s0.copy()
    u1[1], s1[1] = wide_oracle_values(whole, nano)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_snapshot_update_wide(9549, 9551, [1], whole, nano, pres[1])
    assert e.value.code == ESTALE
    bad = nano.copy()
    bad[5] = 10**9
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_snapshot_update_wide(9550, 9551, [1], whole, bad, pres[1])
    assert e.value.code == EINVAL
    assert ctx.tas_snapshot_info()[0] == 9550 and ctx.tas_snapshot_wide_count() == 0
    ctx.tas_snapshot_update_wide(9550, 9551, [1], whole, nano, pres[1])
    assert ctx.tas_snapshot_wide_count() == 1
    check(9551, u1, s1)
    # set_scale ignores the wide column's entry; the others move
    ctx.tas_snapshot_set_scale(9551, [3, 9, 0])
    check(9551, u1, s1)
    # the top-k entry points refuse a snapshot with a wide column
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    k, P = 8, len(prio)
    key = torch.empty((P, k), dtype=torch.int64, device="cuda")
    node = torch.empty((P, k), dtype=torch.int32, device="cuda")
    ln = torch.empty(P, dtype=torch.int32, device="cuda")
    topk_args = (P, len(rules), dev(rules.view(np.uint8)), dev(off), dev(prio.view(np.uint8)),
                 None, k, 0, key, node, ln)
    from pas_amd import workload as wl
    gs = wl.make_gas_snapshot(N, seed=3)
    gb = wl.make_gas_batch(P, seed=3)
    ctx.gas_snapshot_set(9559, gs.n_cards, gs.cap, gs.used)
    gas_args = (P, len(rules), dev(rules.view(np.uint8)), dev(off), dev(prio.view(np.uint8)),
                None, gb.req.shape[1], wl.I915, dev(gb.req), dev(gb.req_mask.view(np.int32)),
                dev(gb.n_containers), k, 0, key, node, ln)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_topk_device(9551, *topk_args)
    assert e.value.code == ENOTEXACT and "column 1" in str(e.value)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_gas_topk_device(9551, 9559, *gas_args)
    assert e.value.code == ENOTEXACT and "column 1" in str(e.value)
    # the device form, with a nano past the range read clamped
    w2, n2 = random_wide(rng, N)
    n2_in = n2.copy()
    n2_in[7] = 2 * 10**9
    w2[7], n2[7] = 3, 999_999_999
    ctx.tas_snapshot_update_wide_device(9551, 9552, [1], dev(w2), dev(n2_in.view(np.int32)),
                                        dev(pres[1].view(np.int64)))
    ctx.synchronize()
    u1[1], s1[1] = wide_oracle_values(w2, n2)
    check(9552, u1, s1)
    # wide -> narrow: a plain update returns the column to its recorded scale (4)
    v2 = rng.integers(-30000, 30000, N).astype(np.int64)
    ctx.tas_snapshot_update(9552, 9553, [1], v2, pres[1])
    assert ctx.tas_snapshot_wide_count() == 0
    u2, s2 = v.copy(), s0.copy()
    u2[1] = v2
    check(9553, u2, s2)
    # the top-k entry points answer again: the first k of each pod's list
    ctx.tas_topk_device(9553, *topk_args)
    ctx.synchronize()
    _, wo, wlens = oracle.tas_eval(u2, pres, rules, off, prio, v_scale=s2)
    got_n, got_l = node.cpu().numpy(), ln.cpu().numpy()
    for p in range(P):
        m = min(k, int(wlens[p]))
        assert got_l[p] == m
        np.testing.assert_array_equal(got_n[p, :m], wo[p, :m])
    # wide again, then a whole set: every column narrow (milli)
    ctx.tas_snapshot_update_wide(9553, 9554, [0, 2], np.stack([whole, w2]),
                                 np.stack([nano, n2]), pres[[0, 2]])
    assert ctx.tas_snapshot_wide_count() == 2
    ctx.tas_snapshot_set(9555, v, pres)
    assert ctx.tas_snapshot_wide_count() == 0
    check(9555, v, np.full((M, N), 3, np.int8))
    ctx.tas_topk_device(9555, *topk_args)
    ctx.tas_gas_topk_device(9555, 9559, *gas_args)
    ctx.synchronize()


@pytest.mark.gpu
def test_set_wide_failure_leaves_no_snapshot(ctx):
    v = np.zeros((1, 4), np.int64)
    pres = pack_bits(np.ones((1, 4), bool))
    wide = {0: (np.arange(4, dtype=np.int64), np.array([0, 1, 10**9, 2], np.uint32))}
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_snapshot_set_wide(9560, v, pres, [3], wide)
    assert e.value.code == EINVAL
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_snapshot_info()
    assert e.value.code == pas_amd._lib.PAS_ENOSNAP


@pytest.mark.gpu
def test_extender_mirror(ctx):
    from pas_amd import extender as ext
    from pas_amd import wire
    nodes, metrics, names = PAST_CASE
    v, pres, scale, wide = sn.tas_snapshot_from_metrics_wide(metrics, nodes, names)
    ctx.tas_snapshot_set_wide(9570, v, pres, scale, wide)
    rs = Restated(decimal_matrix(metrics, nodes, names))
    policies = {("default", "p"): {"scheduleonmetric": [("past", "GreaterThan", 0)],
                                   "dontschedule": [("past", "GreaterThan", 9 * 10**18),
                                                    ("past", "Equals", 1000000000000),
                                                    ("past", "LessThan", -9 * 10**18)]},
                ("default", "q"): {"scheduleonmetric": [("past", "LessThan", 0)],
                                   "dontschedule": [("past", "Equals", 4611686018427387904)]}}
    m = ext.MetricsExtender(ctx, 9570, nodes, names, policies)
    rng = np.random.default_rng(0x6)
    req_names = [nodes[i] for i in rng.permutation(len(nodes))] + [nodes[3], "stranger"]
    idx = np.array([nodes.index(n) if n in nodes else -1 for n in req_names], np.int32)

    def body(policy):
        item = lambda n: {"metadata": {"name": n}, "spec": {}, "status": {}}  # noqa: E731
        return json.dumps({"Pod": {"metadata": {"name": "pod", "namespace": "default",
                                                "labels": {"telemetry-policy": policy}}},
                           "Nodes": {"metadata": {}, "items": [item(n) for n in req_names]},
                           "NodeNames": req_names}).encode()

    for policy, ops in (("p", 1), ("q", 0)):
        status, got = m.prioritize(body(policy))
        pos = rs.prioritize_request(np.array([(0, ops, 0)], RULE_DTYPE)[0], idx)
        assert status == 200 and got == wire.host_priority_list(pos, wire.NodeTable(req_names))
        assert [h["Host"] for h in json.loads(got)] == [req_names[j] for j in pos]
        status, got = m.filter(body(policy))
        triples = policies[("default", policy)]["dontschedule"]
        rules = np.array([(0, pas_amd.parse_operator(o), t) for _, o, t in triples], RULE_DTYPE)
        viol = unpack_bits(rs.tas_violations(rules, np.array([0, len(rules)], np.int32)),
                           len(nodes))[0]
        res = json.loads(got)
        assert status == 200
        want_failed = {n for n in req_names if n in nodes and viol[nodes.index(n)]}
        assert set(res["FailedNodes"]) == want_failed
        assert [it["metadata"]["name"] for it in res["Nodes"]["items"] or []] == \
            [n for n in req_names if n not in want_failed]
