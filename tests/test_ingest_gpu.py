"""Quantity literals parsed on the device (csrc/tas_ingest.hip): the batch parse against the
host parser, and the column refresh from literals against today's path (the host builder
snapshot.tas_snapshot_from_metrics_wide + pas_tas_snapshot_update + _update_wide + _set_scale)
applied to the same base snapshot.  The yardsticks are the host functions of quantity.cpp,
that path and the oracle, never the new code."""
import random

import numpy as np
import pytest
import torch

import pas_amd
import quantity_corpus as qc
from helpers import RULE_DTYPE, unpack_bits
from pas_amd import _lib
from pas_amd import snapshot as sn
from pas_amd.workload import pack_bits
from test_wide_columns import OracleChecker

pytestmark = pytest.mark.gpu
OK, EINVAL, ENOTEXACT = _lib.PAS_OK, _lib.PAS_EINVAL, _lib.PAS_ENOTEXACT
DEV = "cuda:0"


# ------------------------------------------------------------------ batch parse
def check_batch(got, refs):
    whole, nano, dec, status = got
    assert len(status) == len(refs)
    for i, r in enumerate(refs):
        assert (int(status[i]), int(whole[i]), int(nano[i])) == r[:3], (i, r)
        if r[0] != EINVAL:
            assert int(dec[i]) == r[3], (i, r)


def parse_device(ctx, off, blob, n_bytes=None, pad=0):
    """The _device form; the blob sits `pad` bytes inside an allocation of digit bytes."""
    n = len(off) - 1
    big = torch.full((pad + max(len(blob), 1) + pad,), ord("7"), dtype=torch.uint8, device=DEV)
    if blob:
        big[pad:pad + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    off_t = torch.tensor(list(off), dtype=torch.int64, device=DEV)
    whole = torch.full((max(n, 1),), -7, dtype=torch.int64, device=DEV)
    nano = torch.full((max(n, 1),), 7, dtype=torch.int32, device=DEV)
    dec = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    status = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    ctx.quantities_to_wide_device(n, len(blob) if n_bytes is None else n_bytes, off_t, big[pad:],
                                  whole, nano, dec, status)
    ctx.synchronize()
    return (whole.cpu().numpy()[:n], nano.cpu().numpy().view(np.uint32)[:n],
            dec.cpu().numpy()[:n], status.cpu().numpy()[:n])


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, None])
def test_batch_parse_corpus(ctx, n):
    lits, refs = qc.corpus()
    lits, refs = lits[:n], refs[:n]
    off, blob = qc.pack(lits)
    check_batch(ctx.quantities_to_wide(off, blob), refs)
    check_batch(parse_device(ctx, off, blob), refs)


def test_batch_parse_lengths_1_to_200(ctx):
    rng = random.Random(200)
    lits = []
    for length in range(1, 201):
        d = "".join(rng.choice("0123456789") for _ in range(length))
        lits.append(d)
        if length >= 3:
            lits.append("0." + d[2:])
            cut = rng.randint(1, length - 2)
            lits.append(d[:cut] + "." + d[cut + 1:])
        if length >= 5:
            lits.append("-." + d[4:] + rng.choice(["Ki", "Mi", "Ei"]))
            lits.append(d[:length - 4] + "e-" + "%02d" % rng.randint(0, 99))
    assert {len(l) for l in lits} == set(range(1, 201))
    refs = [qc.host_reference(l) for l in lits]
    off, blob = qc.pack(lits)
    check_batch(ctx.quantities_to_wide(off, blob), refs)
    check_batch(parse_device(ctx, off, blob), refs)


def test_batch_parse_specials(ctx):
    """The quirk list, the hand-pinned exponents, an empty literal and bytes 0 in one batch."""
    lits = [q[0] for q in qc.QUIRKS] + [h[0] for h in qc.HUGE_EXPONENT] + [b""] + qc.NUL_INSIDE
    refs = [qc.host_reference(q[0]) for q in qc.QUIRKS] + [h[1] for h in qc.HUGE_EXPONENT]
    refs += [(EINVAL, 0, 0, 0, -1)] * (1 + len(qc.NUL_INSIDE))
    off, blob = qc.pack(lits)
    check_batch(ctx.quantities_to_wide(off, blob), refs)
    check_batch(parse_device(ctx, off, blob), refs)


def test_batch_parse_host_form_checks_offsets(ctx):
    for off in ([1, 2], [0, 3, 2], [0, -1]):
        with pytest.raises(pas_amd.PasError) as e:
            ctx.quantities_to_wide(off, b"123")
        assert e.value.code == EINVAL


def test_batch_parse_device_form_clamps_offsets(ctx):
    """Offsets that are not monotone or point outside [0, n_bytes]: every span is read clamped.
    The blob's surroundings hold digit bytes, so a missing clamp is a wrong value."""
    blob = b"12.5" + b"3Ki" + b"1e3" + b"250m"
    n_bytes = len(blob)
    off = [0, 4, 7, 10, 14, 2, -5, 3, n_bytes + 50, n_bytes + 60, 10, 4, 4, -9, -3, 7, 1 << 40,
           -(1 << 40), 14, 0]
    refs = []
    for i in range(len(off) - 1):
        b = min(max(off[i], 0), n_bytes)
        e = max(min(max(off[i + 1], 0), n_bytes), b)
        refs.append(qc.host_reference(blob[b:e].decode()) if e > b else (EINVAL, 0, 0, 0, -1))
    assert sum(r[0] == EINVAL for r in refs) >= 5 and sum(r[0] == OK for r in refs) >= 5
    check_batch(parse_device(ctx, off, blob, pad=4096), refs)
    # n_bytes below the blob's length is the bound
    refs3 = [qc.host_reference("12."), (EINVAL, 0, 0, 0, -1)]
    check_batch(parse_device(ctx, [0, 9, 12], blob, n_bytes=3, pad=4096), refs3)


# ------------------------------------------------------------------ columns
M_BASE = 16
BACK = 5  # wide in the base snapshot, refreshed back to narrow


def base_snapshot(n, seed=1):
    """Narrow milli columns with random presence, column BACK wide, column 7 at scale 5."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-10**6, 10**6, (M_BASE, n)).astype(np.int64)
    p = pack_bits(rng.random((M_BASE, n)) < 0.7)
    scale = np.full(M_BASE, 3, np.int32)
    scale[7] = 5
    whole = rng.integers(-2**62, 2**62, n).astype(np.int64)
    nano = rng.integers(0, 10**9, n).astype(np.uint32)
    v[BACK] = 0
    return v, p, scale, {BACK: (whole, nano)}


def set_base(ctx, gen, base):
    ctx.tas_snapshot_set_wide(gen, *base)


def todays_path(ctx, gen, metrics, node_names, order, cols):
    """The builder and the three calls TasCache._flush issues; returns (gen, scale, wide)."""
    v, p, scale, wide = sn.tas_snapshot_from_metrics_wide(metrics, node_names, order)
    narrow = [j for j in range(len(order)) if j not in wide]
    if narrow:
        ctx.tas_snapshot_update(gen, gen + 1, [cols[j] for j in narrow], v[narrow], p[narrow])
        gen += 1
    if wide:
        js = sorted(wide)
        ctx.tas_snapshot_update_wide(gen, gen + 1, [cols[j] for j in js],
                                     np.stack([wide[j][0] for j in js]),
                                     np.stack([wide[j][1] for j in js]), p[js])
        gen += 1
    full = ctx.tas_snapshot_get()[3].copy()
    for j in narrow:
        full[cols[j]] = scale[j]
    ctx.tas_snapshot_set_scale(gen, full)
    return gen, scale, wide


def assert_same_snapshot(a, b, only_scale_of=None):
    """Two pas_tas_snapshot_get results: present bits, values and nanos where present, wide
    marks, and the scales of the narrow columns."""
    _, va, pa, sa, wa, na = a
    _, vb, pb, sb, wb, nb = b
    np.testing.assert_array_equal(pa, pb)
    np.testing.assert_array_equal(wa, wb)
    bits = unpack_bits(pa, va.shape[1])
    np.testing.assert_array_equal(va[bits], vb[bits])
    np.testing.assert_array_equal(na[bits], nb[bits])
    narrow = wa == 0
    np.testing.assert_array_equal(sa[narrow], sb[narrow])


def ok_literals(k, seed):
    lits, refs = qc.corpus()
    ok = [l for l, r in zip(lits, refs) if r[0] == OK]
    return random.Random(seed).sample(ok, k)


def column_cases(n):
    """({metric: {node: literal}}, node_index with out-of-range ghosts, expectations)."""
    nodes = [f"n{i}" for i in range(n)]

    def cyc(vals, step=1):
        return {nodes[i]: vals[i % len(vals)] for i in range(0, n, step)}

    metrics = {
        "milli": cyc(["1", "2.5", "100m"]),
        "e7": cyc(["1e-7", "1"]),
        "mix": cyc(["1e-7", "1e12"]),
        "big": {nodes[n // 2]: "1e16"},
        "max": cyc(["9223372036854775807"], 3),
        "ties": cyc(["-0.5", "-0.5", "0", "+"]),
        "empty": {},
        "outside": {f"ghost{i}": lit for i, lit in enumerate(["1", "1e-9", "1e16", "7Ki"])},
        "back": cyc(["3", "4"]),
    }
    rng = random.Random(n)
    for r in range(3):
        lits = ok_literals(n, 100 * n + r)
        metrics[f"rand{r}"] = {nodes[i]: lits[i] for i in range(n) if rng.random() < 0.8}
        metrics[f"rand{r}"]["ghost0"] = "5"
    index = {name: i for i, name in enumerate(nodes)}
    index.update({"ghost0": -1, "ghost1": n, "ghost2": n + 1000, "ghost3": -2**31})
    # (kind, scale) the issue states, where the column has the nodes for it
    expect = {"milli": (0, 3), "e7": (0, 7), "big": (1, None), "max": (1, None), "ties": (0, 3),
              "empty": (0, 3), "outside": (0, 3), "back": (0, 3)}
    if n >= 2:
        expect["mix"] = (1, None)
    return nodes, metrics, index, expect


COLS = {"milli": 0, "e7": 9, "mix": 2, "big": 11, "max": 4, "ties": 15, "empty": 6, "outside": 7,
        "back": BACK, "rand0": 13, "rand1": 1, "rand2": 10}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_columns_equal_todays_path(ctx, n):
    nodes, metrics, index, expect = column_cases(n)
    order = ["ties", "rand1", "milli", "outside", "mix", "rand0", "back", "e7", "empty", "max",
             "rand2", "big"]  # cols not ascending
    cols = [COLS[name] for name in order]
    assert sorted(cols) != cols and len(set(cols)) == len(cols)
    base = base_snapshot(n)
    gen = 7000 + 10 * n
    set_base(ctx, gen, base)
    before = ctx.tas_snapshot_get()
    gen_a, b_scale, b_wide = todays_path(ctx, gen, metrics, nodes, order, cols)
    want = ctx.tas_snapshot_get()
    untouched = [m for m in range(M_BASE) if m not in cols]
    np.testing.assert_array_equal(want[2][untouched], before[2][untouched])

    packed = sn.pack_quantities(metrics, index, order)
    for form in ("host", "device"):
        set_base(ctx, gen, base)
        if form == "host":
            kind, scale = ctx.tas_snapshot_update_quantities(gen, gen + 5, cols, *packed)
        else:
            col_off, entry_node, lit_off, blob = packed
            kind, scale = ctx.tas_snapshot_update_quantities_device(
                gen, gen + 5, cols, col_off, len(blob),
                torch.from_numpy(entry_node).to(DEV), torch.from_numpy(lit_off).to(DEV),
                torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV))
        got = ctx.tas_snapshot_get()
        assert got[0] == gen + 5
        assert_same_snapshot(got, want)
        # what the call did not name is as the base had it
        np.testing.assert_array_equal(got[1][untouched], before[1][untouched])
        np.testing.assert_array_equal(got[3][untouched], before[3][untouched])
        for j, name in enumerate(order):
            assert int(kind[j]) == (j in b_wide), (form, name)
            if j not in b_wide:
                assert int(scale[j]) == int(b_scale[j]), (form, name)
            else:  # a wide column keeps the scale recorded before
                assert int(scale[j]) == int(before[3][cols[j]]), (form, name)
            if name in expect:
                assert int(kind[j]) == expect[name][0], (form, name)
                if expect[name][1] is not None:
                    assert int(scale[j]) == expect[name][1], (form, name)
        assert ctx.tas_snapshot_wide_count() == len(b_wide)


# ------------------------------------------------------------------ evaluation, policy table
EVAL_COLS = {
    "milli": ["1", "2.5", "100m", "3", "-2"],
    "e7": ["1e-7", "1", "2", "-1e-7", "0"],
    "mix": ["1e-7", "1e12", "3", "-1e12", "2"],
    "big": ["1e16", "1", "-1e16", "2"],
    "max": ["9223372036854775807", "-9223372036854775807", "0", "1"],
    "ties": ["-0.5", "-0.5", "0", "+"],
}
EVAL_TARGETS = [-3, -2, -1, 0, 1, 2, 3, 10**12, 10**16, 2**63 - 1, -(2**63 - 1), -2**63]


def oracle_arrays(metrics, nodes, names):
    """The oracle's per-value decimal form from the host parser: u = value * 10^s exactly at the
    value's own decimal places s (every literal here fits int64 there), and presence."""
    m, n = len(names), len(nodes)
    u = np.zeros((m, n), np.int64)
    s = np.zeros((m, n), np.int8)
    pres = np.zeros((m, n), bool)
    for j, name in enumerate(names):
        for i, node in enumerate(nodes):
            if node in metrics[name]:
                s[j, i] = pas_amd.quantity_decimals(metrics[name][node])
                u[j, i] = pas_amd.quantity_to_scaled(metrics[name][node], int(s[j, i]))
                pres[j, i] = True
    return u, s, pack_bits(pres)


def eval_case(n=130):
    nodes = [f"n{i}" for i in range(n)]
    rng = random.Random(5)
    metrics = {name: {nodes[i]: vals[i % len(vals)] for i in range(n) if rng.random() < 0.85}
               for name, vals in EVAL_COLS.items()}
    return nodes, metrics, list(EVAL_COLS)


def eval_rules(m):
    """One single-rule pod per (metric, LessThan / GreaterThan / Equals, target), prioritized
    by the same metric and operator; then pods of three rules."""
    rules = [(c, op, t) for c in range(m) for op in range(3) for t in EVAL_TARGETS]
    off = list(range(len(rules) + 1))
    prio = [(c, op, 0) for c, op, _ in rules]
    rng = np.random.default_rng(0x16)
    for _ in range(32):
        for _ in range(3):
            rules.append((int(rng.integers(0, m)), int(rng.integers(0, 3)),
                          int(EVAL_TARGETS[int(rng.integers(0, len(EVAL_TARGETS)))])))
        off.append(len(rules))
        prio.append((int(rng.integers(0, m)), int(rng.integers(0, 3)), 0))
    return (np.array(rules, RULE_DTYPE), np.array(off, np.int32), np.array(prio, RULE_DTYPE))


def test_evaluation_after_refresh(ctx, oracle):
    nodes, metrics, names = eval_case()
    n, m = len(nodes), len(names)
    empty = (np.zeros((m, n), np.int64), np.zeros((m, (n + 63) // 64), np.uint64))
    cols = list(range(m))
    rules, off, prio = eval_rules(m)
    cand = pack_bits(np.random.default_rng(3).random((len(prio), n)) < 0.9)

    ctx.tas_snapshot_set(7700, *empty)
    gen, _, wide = todays_path(ctx, 7700, metrics, nodes, names, cols)
    assert sorted(wide) == [names.index(c) for c in ("mix", "big", "max")]
    want = ctx.tas_eval(gen, rules, off, prio, cand)

    ctx.tas_snapshot_set(7700, *empty)
    index = {name: i for i, name in enumerate(nodes)}
    ctx.tas_snapshot_update_quantities(7700, 7701, cols, *sn.pack_quantities(metrics, index, names))
    got = ctx.tas_eval(7701, rules, off, prio, cand)
    # byte-equal: the pass words, the lengths, and every list (a row is defined up to its length)
    assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert int(want[2].max()) > 50 and int(want[2].min()) == 0
    for p in range(len(prio)):
        assert got[1][p, :want[2][p]].tobytes() == want[1][p, :want[2][p]].tobytes(), p
    # and the oracle, per value at its own decimal places
    u, s, opres = oracle_arrays(metrics, nodes, names)
    wp, wo, wl = OracleChecker(oracle, u, s, opres).tas_eval(rules, off, prio, cand)
    np.testing.assert_array_equal(got[0], wp)
    np.testing.assert_array_equal(got[2], wl)
    for p in range(len(wl)):
        np.testing.assert_array_equal(got[1][p, :wl[p]], wo[p, :wl[p]], err_msg=f"pod {p}")


def test_policy_table_reflects_refresh(ctx, oracle):
    nodes, metrics, names = eval_case(65)
    n, m = len(nodes), len(names)
    index = {name: i for i, name in enumerate(nodes)}
    ctx.tas_snapshot_set(7800, np.zeros((m, n), np.int64), np.zeros((m, 2), np.uint64))
    ctx.tas_snapshot_update_quantities(7800, 7801, list(range(m)),
                                       *sn.pack_quantities(metrics, index, names))
    rules, off, prio = eval_rules(m)
    rules, off, prio = rules[:off[60]], off[:61], prio[:60]
    ctx.tas_policies_set(rules, off, prio)
    try:
        u, s, opres = oracle_arrays(metrics, nodes, names)
        first = ctx.tas_policies_violated(7801)
        np.testing.assert_array_equal(
            first, OracleChecker(oracle, u, s, opres).tas_violations(rules, off))
        # every value of two columns changes: a narrow column to other values at another scale,
        # a wide column to narrow
        metrics2 = dict(metrics)
        metrics2["milli"] = {node: "2.00001" for node in nodes[::2]}
        metrics2["big"] = {node: "-1" for node in nodes}
        changed = ["big", "milli"]
        kind, scale = ctx.tas_snapshot_update_quantities(
            7801, 7802, [names.index(c) for c in changed],
            *sn.pack_quantities(metrics2, index, changed))
        assert kind.tolist() == [0, 0] and scale.tolist() == [3, 5]
        u, s, opres = oracle_arrays(metrics2, nodes, names)
        second = ctx.tas_policies_violated(7802)
        np.testing.assert_array_equal(
            second, OracleChecker(oracle, u, s, opres).tas_violations(rules, off))
        assert not np.array_equal(first, second)
    finally:
        ctx.tas_policies_drop()


# ------------------------------------------------------------------ failures change nothing
def snapshot_bytes(ctx):
    return [np.asarray(x).tobytes() for x in ctx.tas_snapshot_get()]


@pytest.mark.parametrize("lits,nodes,code,at", [
    (["1", "2", "1e19", "3"], [0, 1, 2, 3], ENOTEXACT, 2),
    (["1", "1K", "3", "1e19"], [0, 1, 2, 3], EINVAL, 1),
    (["1", "1e19", "1K"], [0, 1, 2], ENOTEXACT, 1),
    (["1", "2", "3", "1K"], [0, 1, 2, -1], EINVAL, 3),       # the bad entry's node out of range
    (["1", "2", "3", "1e19"], [0, 1, 2, 10**6], ENOTEXACT, 3),
    (["1", "", "3"], [0, 1, 2], EINVAL, 1),
])
@pytest.mark.parametrize("form", ["host", "device"])
def test_all_or_nothing(ctx, lits, nodes, code, at, form):
    base = base_snapshot(65, seed=4)
    set_base(ctx, 7900, base)
    before = snapshot_bytes(ctx)
    # two columns: a good one first, so the bad entry's index is not its index in its column
    good = ["7", "8.5"]
    off, blob = qc.pack(good + lits)
    col_off = np.array([0, len(good), len(good) + len(lits)], np.int64)
    entry_node = np.array([3, 4] + nodes, np.int32)
    lit_off = np.array(off, np.int64)
    with pytest.raises(pas_amd.PasError) as e:
        if form == "host":
            ctx.tas_snapshot_update_quantities(7900, 7901, [2, BACK], col_off, entry_node,
                                               lit_off, blob)
        else:
            ctx.tas_snapshot_update_quantities_device(
                7900, 7901, [2, BACK], col_off, len(blob), torch.from_numpy(entry_node).to(DEV),
                torch.from_numpy(lit_off).to(DEV),
                torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV))
    assert e.value.code == code
    assert e.value.bad_entry == len(good) + at
    assert snapshot_bytes(ctx) == before  # generation, values, presence, scales, marks, nanos
    assert ctx.tas_snapshot_wide_count() == 1


# ------------------------------------------------------------------ duplicates
def test_duplicates(ctx):
    n = 65
    base = base_snapshot(n, seed=6)
    set_base(ctx, 8000, base)
    before = snapshot_bytes(ctx)
    # column 3: node 0 twice, the loser has the most decimals; column 8: node 64 twice, the
    # loser does not fit milli
    lits = ["1e-7", "2", "1", "1e16", "5", "6"]
    nodes = [0, 1, 0, 64, 64, 2]
    off, blob = qc.pack(lits)
    col_off = np.array([0, 3, 6], np.int64)
    entry_node = np.array(nodes, np.int32)
    lit_off = np.array(off, np.int64)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_snapshot_update_quantities(8000, 8001, [3, 8], col_off, entry_node, lit_off, blob)
    assert e.value.code == EINVAL and e.value.bad_entry == -1
    assert snapshot_bytes(ctx) == before
    # the same node in two different columns is no duplicate; neither is an out-of-range node
    ctx.tas_snapshot_update_quantities(8000, 8001, [3, 8], np.array([0, 2, 5], np.int64),
                                       np.array([0, 1, 0, -1, -1], np.int32),
                                       np.array(qc.pack(lits[:5])[0], np.int64),
                                       qc.pack(lits[:5])[1])
    set_base(ctx, 8000, base)
    kind, scale = ctx.tas_snapshot_update_quantities_device(
        8000, 8001, [3, 8], col_off, len(blob), torch.from_numpy(entry_node).to(DEV),
        torch.from_numpy(lit_off).to(DEV),
        torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV))
    # the highest index gives the value; scale and kind count every in-range entry
    assert kind.tolist() == [0, 1] and int(scale[0]) == 7
    _, v, p, s, w, nano = ctx.tas_snapshot_get()
    assert np.flatnonzero(unpack_bits(p[3:4], n)[0]).tolist() == [0, 1]
    assert v[3, 0] == 1 * 10**7 and v[3, 1] == 2 * 10**7 and s[3] == 7 and w[3] == 0
    assert np.flatnonzero(unpack_bits(p[8:9], n)[0]).tolist() == [2, 64]
    assert (v[8, 64], nano[8, 64]) == (5, 0) and (v[8, 2], nano[8, 2]) == (6, 0) and w[8] == 1


# ------------------------------------------------------------------ generations and arguments
def test_generations_and_arguments(ctx):
    base = base_snapshot(64, seed=8)
    set_base(ctx, 8100, base)
    one = (np.array([0, 1], np.int64), np.array([0], np.int32), np.array([0, 1], np.int64), b"1")
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_snapshot_update_quantities(8099, 8101, [0], *one)
    assert e.value.code == _lib.PAS_ESTALE
    for cols in ([0, 0], [0, M_BASE], [-1, 0]):  # repeated, outside the snapshot
        two = (np.array([0, 1, 1], np.int64),) + one[1:]
        with pytest.raises(pas_amd.PasError) as e:
            ctx.tas_snapshot_update_quantities(8100, 8101, cols, *two)
        assert e.value.code == EINVAL
    for col_off in ([1, 1], [0, 2]):  # col_off not from 0; lit_off decreasing
        with pytest.raises(pas_amd.PasError) as e:
            ctx.tas_snapshot_update_quantities(8100, 8101, [0], np.array(col_off, np.int64),
                                               np.array([0, 0], np.int32),
                                               np.array([0, 1, 0], np.int64), b"1")
        assert e.value.code == EINVAL
    before = snapshot_bytes(ctx)
    # n_cols = 0 moves the generation only
    none = (np.array([0], np.int64), np.zeros(0, np.int32), np.array([0], np.int64), b"")
    kind, scale = ctx.tas_snapshot_update_quantities(8100, 8200, [], *none)
    assert len(kind) == 0 and len(scale) == 0
    after = snapshot_bytes(ctx)
    assert ctx.tas_snapshot_info()[0] == 8200 and after[1:] == before[1:]
    kind, _ = ctx.tas_snapshot_update_quantities_device(8200, 8201, [], np.array([0], np.int64),
                                                        0, None, None, None)
    assert ctx.tas_snapshot_info()[0] == 8201
    # no snapshot
    ctx._l.pas_tas_snapshot_drop(ctx._h)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_snapshot_update_quantities(8201, 8202, [0], *one)
    assert e.value.code == _lib.PAS_ENOSNAP
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_snapshot_update_quantities_device(8201, 8202, [], np.array([0], np.int64), 0,
                                                  None, None, None)
    assert e.value.code == _lib.PAS_ENOSNAP
