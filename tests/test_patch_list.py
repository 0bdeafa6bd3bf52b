"""The deschedule label plan as a compact patch list (pas_tas_label_patches,
pas_tas_deschedule_patches, DescheduleEnforcer.enforce_changes): only the nodes whose PATCH body
is not "[]", in ascending node index, optionally without what would write a value the label
already has.

Expected values: the oracle's plan (oracle.label_plan: add, rem, total) and the definitions of
include/pas.h restated in numpy below (`reduce_masks`, then np.nonzero(add | rem)).

Launch boundaries of tas_patches.hip: a word is 64 nodes, a segment 1024 nodes (one workgroup of
four waves, four words each), the scan takes 256 segments per chunk: node counts around 64 and
1024, several segments, and one size past 256 segments (the scan's second chunk and carry)."""
import numpy as np
import pytest
import torch

import pas_amd
from pas_amd import workload as wl
from pas_amd.extender import DescheduleEnforcer
from helpers import NamedSnapshot, golden, unpack_bits
from test_labels import name_labels, random_names
from test_oracle_golden import apply_label_patch, g4n_inputs

pytestmark = pytest.mark.gpu

G = golden()
EINVAL, ESTALE, ENOSNAP = (pas_amd._lib.PAS_EINVAL, pas_amd._lib.PAS_ESTALE,
                           pas_amd._lib.PAS_ENOSNAP)
SENTINEL = 0x5A5A5A5A


def first_strategy(names, s):
    """k[s]: the first strategy with the name of s."""
    if names is None:
        return list(range(s))
    return [names.index(x) for x in names]


def reduce_masks(add, rem, n, labels, violating, null, names):
    """add' and rem' of pas.h from the plan's masks and the value bitmaps."""
    add, rem = add.copy(), rem.copy()
    s = 0 if labels is None else labels.shape[0]
    if labels is None or s == 0 or n == 0:
        return add, rem
    first = first_strategy(names, s)
    carried = unpack_bits(labels, n)
    for k in sorted(set(first)):
        members = np.uint64(sum(1 << j for j in range(s) if first[j] == k))
        if violating is not None:
            add[carried[k] & unpack_bits(violating[k:k + 1], n)[0]] &= ~members
        if null is not None:
            rem[carried[k] & unpack_bits(null[k:k + 1], n)[0]] &= ~np.uint64(1 << k)
    return add, rem


def want_patches(oracle, viol, n, labels=None, names=None, violating=None, null=None):
    """(node, add', rem', total) of the definitions."""
    add, rem, total = oracle.label_plan(viol, labels, n, names)
    add, rem = reduce_masks(add, rem, n, labels, violating, null, names)
    node = np.nonzero(add | rem)[0]
    return node.astype(np.int32), add[node], rem[node], total


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype.fields:
        a = a.view(np.uint8)
    return torch.from_numpy(a.copy()).cuda()


class DeviceRecords:
    """Record arrays of cap + pad entries filled with a sentinel, and the two counters."""

    def __init__(self, cap, pad=16):
        self.cap = cap
        self.node = torch.full((cap + pad,), SENTINEL, dtype=torch.int32, device="cuda")
        self.add = torch.full((cap + pad,), SENTINEL, dtype=torch.int64, device="cuda")
        self.rem = torch.full((cap + pad,), SENTINEL, dtype=torch.int64, device="cuda")
        self.n = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        self.total = torch.full((1,), -7, dtype=torch.int64, device="cuda")

    def check(self, want, what):
        """The first min(cap, n) records exact, everything past them the sentinel, n full."""
        torch.cuda.synchronize()
        w_node, w_add, w_rem, w_total = want
        k = min(self.cap, len(w_node))
        assert int(self.n.item()) == len(w_node), what
        assert int(self.total.item()) == w_total, what
        node = self.node.cpu().numpy()
        add = self.add.cpu().numpy().view(np.uint64)
        rem = self.rem.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(node[:k], w_node[:k], err_msg=f"node {what}")
        np.testing.assert_array_equal(add[:k], w_add[:k], err_msg=f"add {what}")
        np.testing.assert_array_equal(rem[:k], w_rem[:k], err_msg=f"rem {what}")
        assert np.all(node[k:] == SENTINEL) and np.all(add[k:] == SENTINEL) and \
            np.all(rem[k:] == SENTINEL), f"written past the list: {what}"


def check_host(got, want, what):
    node, add, rem, n, total = got[:5]
    np.testing.assert_array_equal(node, want[0], err_msg=f"node {what}")
    np.testing.assert_array_equal(add, want[1], err_msg=f"add {what}")
    np.testing.assert_array_equal(rem, want[2], err_msg=f"rem {what}")
    assert n == len(want[0]) and total == want[3], what


def run_both(ctx, oracle, n, viol, labels, names, violating, null, what):
    """The host form and the device form against the definitions."""
    s = viol.shape[0]
    want = want_patches(oracle, viol, n, labels, names, violating, null)
    check_host(ctx.tas_label_patches(n, viol, labels, names, violating, null), want, what)
    rec = DeviceRecords(n)
    ctx.tas_label_patches_device(n, s, dev(viol) if viol.size else None,
                                 dev(labels) if labels is not None and labels.size else None,
                                 dev(violating) if violating is not None and violating.size
                                 else None,
                                 dev(null) if null is not None and null.size else None, n,
                                 rec.node, rec.add, rec.rem, rec.n, rec.total, names=names)
    rec.check(want, what)
    return want


def shared_names(s):
    """One name on three strategies (0, 2 and the last), the others distinct."""
    names = [f"pol-{j}" for j in range(s)]
    names[2] = names[s - 1] = names[0]
    return names


def bitmaps(rng, s, n, density):
    if s == 0 or n == 0:
        return np.zeros((s, (n + 63) // 64), np.uint64)
    return wl.pack_bits(rng.random((s, n)) < density)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_label_patches_parity(ctx, oracle, n):
    rng = np.random.default_rng(5000 + n)
    listed = 0
    for s in (0, 1, 5, 64):
        for names in [None] + ([shared_names(s)] if s >= 5 else []):
            for density in (0.02, 0.3):
                viol = bitmaps(rng, s, n, density)
                labels = bitmaps(rng, s, n, 0.5) if names is None or n == 0 else \
                    name_labels(rng, names, n)
                # independent value bitmaps: bits in both (contradictory input) are common
                violating, null = bitmaps(rng, s, n, 0.5), bitmaps(rng, s, n, 0.5)
                for lab, vio, nul in ((None, None, None), (labels, None, None),
                                      (labels, violating, None), (labels, None, null),
                                      (labels, violating, null), (None, violating, null)):
                    what = f"n={n} s={s} shared={names is not None} d={density} " \
                           f"lab={lab is not None} vio={vio is not None} nul={nul is not None}"
                    listed += len(run_both(ctx, oracle, n, viol, lab, names, vio, nul, what)[0])
    assert listed > 0 or n == 0


def test_label_patches_densities_and_contradiction(ctx, oracle):
    """Nothing listed, every node listed, and value bitmaps of all ones (every carried label
    both "violating" and "null": each bitmap is applied on its own)."""
    n, s = 4097, 5
    names = shared_names(s)
    zeros = np.zeros((s, (n + 63) // 64), np.uint64)
    ones = wl.pack_bits(np.ones((s, n), bool))
    w = run_both(ctx, oracle, n, zeros, None, names, None, None, "all zero")
    assert len(w[0]) == 0 and w[3] == n * 3  # three distinct names, none violated
    w = run_both(ctx, oracle, n, zeros, zeros, names, ones, ones, "no label carried")
    assert len(w[0]) == 0
    w = run_both(ctx, oracle, n, ones, None, names, None, None, "all ones")
    assert len(w[0]) == n and w[3] == 0 and np.all(w[1] == np.uint64(31))
    w = run_both(ctx, oracle, n, zeros, ones, names, None, None, "every label removed")
    assert len(w[0]) == n and np.all(w[2] == np.uint64(0b1011))  # first strategies 0, 1, 3
    # contradictory: everything carried is "violating" and "null": no add, no remove left
    rng = np.random.default_rng(77)
    viol = bitmaps(rng, s, n, 0.3)
    w = run_both(ctx, oracle, n, viol, ones, names, ones, ones, "contradictory")
    assert len(w[0]) == 0
    # the member clearing: a node whose label pol-0 is "violating" keeps no add of strategies
    # 0, 2 and 4, and its other adds
    w = run_both(ctx, oracle, n, ones, ones, names, ones, None, "settled adds")
    assert len(w[0]) == 0
    only0 = zeros.copy()
    only0[0] = ones[0]
    w = run_both(ctx, oracle, n, ones, ones, names, only0, None, "name 0 settled")
    assert len(w[0]) == n and np.all(w[1] == np.uint64(0b01010))


def test_label_patches_past_256_segments(ctx, oracle):
    """257 segments: the scan's second chunk starts from the first one's carry."""
    n, s = 262_144 + 65, 3
    rng = np.random.default_rng(262)
    names = ["a", "b", "a"]
    viol = bitmaps(rng, s, n, 0.3)
    labels = name_labels(rng, names, n)
    violating, null = bitmaps(rng, s, n, 0.5), bitmaps(rng, s, n, 0.5)
    w = run_both(ctx, oracle, n, viol, labels, names, violating, null, "257 segments")
    assert w[0][-1] >= 262_144  # the list reaches the last segment
    run_both(ctx, oracle, n, viol, None, None, None, None, "257 segments, no labels")


def test_label_patches_truncation(ctx, oracle):
    n, s = 4097, 5
    rng = np.random.default_rng(409)
    names = shared_names(s)
    viol = bitmaps(rng, s, n, 0.1)
    labels = name_labels(rng, names, n)
    null = bitmaps(rng, s, n, 0.5)
    want = want_patches(oracle, viol, n, labels, names, None, null)
    n_p = len(want[0])
    assert 100 < n_p < n
    for cap in (0, 1, n_p - 1, n_p, n_p + 7):
        k = min(cap, n_p)
        # host form, the caller's arrays
        out = (np.full(cap + 16, SENTINEL, np.int32), np.full(cap + 16, SENTINEL, np.uint64),
               np.full(cap + 16, SENTINEL, np.uint64))
        node, add, rem, got_n, total = ctx.tas_label_patches(n, viol, labels, names, None, null,
                                                             cap=cap, out=out)
        assert got_n == n_p and total == want[3], cap
        for got, w in ((node, want[0]), (add, want[1]), (rem, want[2])):
            np.testing.assert_array_equal(got[:k], w[:k], err_msg=f"cap={cap}")
            assert np.all(got[k:] == SENTINEL), cap
        # host form, arrays of its own: exactly the records
        got = ctx.tas_label_patches(n, viol, labels, names, None, null, cap=cap)
        assert got[3] == n_p and len(got[0]) == len(got[1]) == len(got[2]) == k
        np.testing.assert_array_equal(got[0], want[0][:k])
        # device form
        rec = DeviceRecords(cap)
        ctx.tas_label_patches_device(n, s, dev(viol), dev(labels), None, dev(null), cap,
                                     rec.node, rec.add, rec.rem, rec.n, rec.total, names=names)
        rec.check(want, f"cap={cap}")
    # counting only: cap 0 and no record arrays
    n_t = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    total_t = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ctx.tas_label_patches_device(n, s, dev(viol), dev(labels), None, dev(null), 0, None, None,
                                 None, n_t, total_t, names=names)
    torch.cuda.synchronize()
    assert int(n_t.item()) == n_p and int(total_t.item()) == want[3]


def test_label_patches_errors(ctx):
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_label_patches(10, np.zeros((65, 1), np.uint64))
    assert e.value.code == EINVAL
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_label_patches(10, np.zeros((2, 1), np.uint64), cap=-1,
                              out=(np.zeros(1, np.int32), np.zeros(1, np.uint64),
                                   np.zeros(1, np.uint64)))
    assert e.value.code == EINVAL
    n_t = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(pas_amd.PasError) as e:  # cap > 0 without record arrays
        ctx.tas_label_patches_device(10, 1, n_t, None, None, None, 4, None, None, None, n_t, n_t)
    assert e.value.code == EINVAL


# ---------------------------------------------------------------- the sweep and the list fused

def fused_all_forms(ctx, oracle, gen, n, rules, off, want_v, labels, names, violating, null,
                    what):
    """pas_tas_deschedule_patches (with and without viol_out) and its device form (the same)
    against the definitions on the oracle's sweep, and against pas_tas_deschedule_device
    followed by the numpy reduction."""
    s = len(off) - 1
    want = want_patches(oracle, want_v, n, labels, names, violating, null)
    check_host(ctx.tas_deschedule_patches(gen, rules, off, labels, names, violating, null), want,
               what)
    got = ctx.tas_deschedule_patches(gen, rules, off, labels, names, violating, null,
                                     want_viol=True)
    check_host(got, want, what)
    np.testing.assert_array_equal(got[5], want_v, err_msg=f"viol_out {what}")
    rules_t, off_t = dev(rules) if len(rules) else None, dev(off)
    d_lab, d_vio, d_nul = (dev(x) if x is not None and x.size else None
                           for x in (labels, violating, null))
    w = (n + 63) // 64
    for with_viol in (False, True):
        rec = DeviceRecords(n)
        viol_t = torch.full((max(s, 1), max(w, 1)), -1, dtype=torch.int64, device="cuda") \
            if with_viol else None
        ctx.tas_deschedule_patches_device(gen, s, len(rules), rules_t, off_t, d_lab, d_vio,
                                          d_nul, viol_t, n, rec.node, rec.add, rec.rem, rec.n,
                                          rec.total, names=names)
        rec.check(want, f"{what} viol_out={with_viol}")
        if with_viol:
            np.testing.assert_array_equal(viol_t.cpu().numpy().view(np.uint64)[:s, :w], want_v)
    # the dense fused call, reduced in numpy
    viol_t = torch.empty((max(s, 1), max(w, 1)), dtype=torch.int64, device="cuda")
    add_t = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    rem_t = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    total_t = torch.empty(1, dtype=torch.int64, device="cuda")
    ctx.tas_deschedule_device(gen, s, len(rules), rules_t, off_t, viol_t, d_lab, add_t, rem_t,
                              total_t, names=names)
    torch.cuda.synchronize()
    add, rem = reduce_masks(add_t.cpu().numpy().view(np.uint64)[:n],
                            rem_t.cpu().numpy().view(np.uint64)[:n], n, labels, violating, null,
                            names)
    node = np.nonzero(add | rem)[0]
    np.testing.assert_array_equal(node, want[0], err_msg=what)
    np.testing.assert_array_equal(add[node], want[1], err_msg=what)
    np.testing.assert_array_equal(rem[node], want[2], err_msg=what)
    assert int(total_t.item()) == want[3], what


@pytest.mark.parametrize("n", [65, 1025, 20_001])
def test_deschedule_patches_parity(ctx, oracle, n):
    rng = np.random.default_rng(6000 + n)
    gen = 7700 + n % 97
    snap = wl.make_tas_snapshot(n, 8, seed=n)
    ctx.tas_snapshot_set(gen, snap.v_milli, snap.present)
    for s in (1, 5, 64):
        rules, off = wl.make_deschedule_rules(snap, s, 2, seed=n + s)
        names = shared_names(s) if s >= 5 else None
        want_v = oracle.tas_violations(snap.v_milli, snap.present, rules, off)
        labels = bitmaps(rng, s, n, 0.4) if names is None else name_labels(rng, names, n, 0.4)
        violating, null = bitmaps(rng, s, n, 0.5), bitmaps(rng, s, n, 0.5)
        for lab, vio, nul in ((None, None, None), (labels, None, None),
                              (labels, violating, null)):
            fused_all_forms(ctx, oracle, gen, n, rules, off, want_v, lab, names, vio, nul,
                            f"n={n} s={s} lab={lab is not None} values={vio is not None}")


def test_deschedule_patches_sub_milli(ctx, oracle):
    from test_submilli_gpu import RANDOM_TARGETS, rule_batch, scaled_snapshot
    rng = np.random.default_rng(0x5B2)
    n, scales = 4097, [0, 3, 4, 6, 9]
    v, pres, u, sc = scaled_snapshot(rng, n, scales)
    ctx.tas_snapshot_set(7800, v, pres, scales)
    rules, off, _ = rule_batch(rng, len(scales), 16, 3, RANDOM_TARGETS)
    want_v = oracle.tas_violations(u, pres, rules, off, v_scale=sc)
    labels = bitmaps(rng, 16, n, 0.4)
    fused_all_forms(ctx, oracle, 7800, n, rules, off, want_v, labels, None,
                    bitmaps(rng, 16, n, 0.5), bitmaps(rng, 16, n, 0.5), "sub-milli")


def test_deschedule_patches_wide_column(ctx, oracle):
    from test_wide_columns import random_wide, rule_batch, wide_oracle_values
    rng = np.random.default_rng(0x2101)
    n, m = 2100, 3
    v = rng.integers(-10**6, 10**6, (m, n)).astype(np.int64)
    pres = wl.pack_bits(rng.random((m, n)) < 0.9)
    u, sc = v.copy(), np.full((m, n), 3, np.int8)
    whole, nano = random_wide(rng, n)
    u[1], sc[1] = wide_oracle_values(whole, nano)
    ctx.tas_snapshot_set(7810, v, pres)
    ctx.tas_snapshot_update_wide(7810, 7811, [1], whole[None], nano[None], pres[[1]])
    assert ctx.tas_snapshot_wide_count() == 1
    targets = sorted({int(x) for x in np.unique(whole[::7])} | {0, 1, -1})
    rules, off, _ = rule_batch(rng, m, 8, 2, targets)
    want_v = oracle.tas_violations(u, pres, rules, off, v_scale=sc)
    labels = bitmaps(rng, 8, n, 0.4)
    fused_all_forms(ctx, oracle, 7811, n, rules, off, want_v, labels, None,
                    bitmaps(rng, 8, n, 0.5), bitmaps(rng, 8, n, 0.5), "wide column")


def test_deschedule_patches_no_strategies_and_errors():
    ctx = pas_amd.Context(0)  # a context of its own: the first call finds no snapshot
    try:
        none = (np.zeros(0, pas_amd.RULE_DTYPE), np.zeros(1, np.int32))
        n_t = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        total_t = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        off_t = torch.zeros(2, dtype=torch.int32, device="cuda")
        with pytest.raises(pas_amd.PasError) as e:
            ctx.tas_deschedule_patches(1, *none)
        assert e.value.code == ENOSNAP
        with pytest.raises(pas_amd.PasError) as e:
            ctx.tas_deschedule_patches_device(1, 0, 0, None, off_t, None, None, None, None, 0,
                                              None, None, None, n_t, total_t)
        assert e.value.code == ENOSNAP
        n = 1000
        snap = wl.make_tas_snapshot(n, 4, seed=3)
        ctx.tas_snapshot_set(7900, snap.v_milli, snap.present)
        node, add, rem, n_p, total = ctx.tas_deschedule_patches(7900, *none)
        assert len(node) == 0 and n_p == 0 and total == 0
        ctx.tas_deschedule_patches_device(7900, 0, 0, None, off_t, None, None, None, None, 0,
                                          None, None, None, n_t, total_t)
        torch.cuda.synchronize()
        assert int(n_t.item()) == 0 and int(total_t.item()) == 0
        # a strategy without rules violates nowhere: nothing listed, every pair counted
        node, add, rem, n_p, total = ctx.tas_deschedule_patches(7900, none[0],
                                                                np.zeros(2, np.int32))
        assert n_p == 0 and total == n
        for gen, s, code in ((7899, 1, ESTALE), (7900, 65, EINVAL)):
            with pytest.raises(pas_amd.PasError) as e:
                ctx.tas_deschedule_patches(gen, none[0], np.zeros(s + 1, np.int32))
            assert e.value.code == code
            with pytest.raises(pas_amd.PasError) as e:
                ctx.tas_deschedule_patches_device(gen, s, 0, None, off_t, None, None, None, None,
                                                  0, None, None, None, n_t, total_t)
            assert e.value.code == code
    finally:
        ctx.close()


# ---------------------------------------------------------------- golden vectors

def test_patches_golden_g4(ctx):
    g = G["G4_deschedule_enforce"]
    snap = NamedSnapshot(g["metrics"], g["nodes"])
    policy = g["policy"]
    n = len(g["nodes"])
    for gen, c in enumerate(g["cases"], start=8000):
        ctx.tas_snapshot_set(gen, snap.v_milli, snap.present)
        rules = snap.rules(c["rules"])
        labels = np.zeros((1, 1), np.uint64)
        if policy in c["labels"]:
            labels[0, 0] = (1 << n) - 1  # every node of this fixture carries c["labels"]
        node, add, rem, n_p, total = ctx.tas_deschedule_patches(
            gen, rules, np.array([0, len(rules)], np.int32), labels)
        assert total == c["derived"]["total"], c["name"]
        masks = {int(i): (a, r) for i, a, r in zip(node, add, rem)}
        a, r = masks.get(0, (0, 0))
        bodies = pas_amd.label_patch_json_batch([policy], [a], [r])
        assert bodies[0].decode() == c["derived"]["patch"], c["name"]
        assert (0 in masks) == (c["derived"]["patch"] != "[]"), c["name"]
        after = {i: apply_label_patch(c["labels"], pas_amd.label_patch_json_batch(
            [policy], [masks.get(i, (0, 0))[0]], [masks.get(i, (0, 0))[1]])[0])
            for i in range(n)}
        assert [x for i, x in enumerate(g["nodes"]) if after[i].get(policy) == "violating"] == \
            c["want"]


def test_patches_golden_g4n(ctx, oracle):
    g = G["G4n_shared_policy_name"]
    snap = NamedSnapshot(g["metrics"], g["nodes"])
    for gen, c in enumerate(g["cases"], start=8100):
        ctx.tas_snapshot_set(gen, snap.v_milli, snap.present)
        names, rules, off, viol_o, labels = g4n_inputs(oracle, c, snap, g["nodes"])
        got = ctx.tas_deschedule_patches(gen, rules, off, labels[:, :1], names)
        node, add, rem, n_p, total = got
        bits = lambda m: [j for j in range(len(names)) if int(m) >> j & 1]  # noqa: E731
        assert total == c["total"], c["name"]
        if c["add"] or c["remove"]:
            assert n_p == 1 and node[0] == 0, c["name"]
            assert bits(add[0]) == c["add"] and bits(rem[0]) == c["remove"], c["name"]
            body = pas_amd.label_patch_json_batch(names, add, rem)[0]
            assert body.decode() == c["patch"], c["name"]
        else:
            assert n_p == 0 and c["patch"] == "[]", c["name"]
        check_host(ctx.tas_label_patches(1, viol_o, labels[:, :1], names),
                   want_patches(oracle, viol_o, 1, labels[:, :1], names), c["name"])


# ---------------------------------------------------------------- the enforcer

def enforcer_case(ctx, gen, n, strategies, seed):
    """A snapshot of metrics m0..m3 over n nodes and the enforcer of `strategies`."""
    rng = np.random.default_rng(seed)
    metric_names = [f"m{j}" for j in range(4)]
    v = rng.integers(0, 100, (4, n)).astype(np.int64) * 1000
    pres = wl.pack_bits(rng.random((4, n)) < 0.95)
    ctx.tas_snapshot_set(gen, v, pres)
    nodes = [f"node-{i}" for i in range(n)]
    return DescheduleEnforcer(ctx, gen, nodes, metric_names, strategies), nodes, rng


def random_labels(rng, names, n):
    """Per node a label dictionary: some strategy names with a value of {"violating", "null",
    "x"}, and an unrelated label."""
    uniq = sorted(set(names))
    out = []
    for _ in range(n):
        lab = {"kubernetes.io/os": "linux"}
        for name in uniq:
            if rng.random() < 0.5:
                lab[name] = ["violating", "null", "x"][int(rng.integers(0, 3))]
        out.append(lab)
    return out


def strategies_for(rng, count, pool):
    """`count` strategies over `pool` policy names (repeats), one or two rules each."""
    ops = ["LessThan", "GreaterThan", "Equals"]
    out = []
    for j in range(count):
        rules = [(f"m{int(rng.integers(0, 4))}", ops[int(rng.integers(0, 3))],
                  int(rng.integers(5, 95))) for _ in range(int(rng.integers(1, 3)))]
        out.append((f"pol-{j % pool}", rules))
    return out


@pytest.mark.parametrize("count,pool", [(5, 3), (64, 40), (150, 100)])
def test_enforce_changes(ctx, count, pool):
    """enforce_changes against enforce: the same non-empty bodies and total; the reduced bodies
    patch every node to the labels the full bodies give; a second pass over the patched labels
    has nothing left to send.  150 strategies: three plan groups merged per node."""
    n = 700
    rng0 = np.random.default_rng(count)
    enf, nodes, rng = enforcer_case(ctx, 8200 + count, n, strategies_for(rng0, count, pool),
                                    seed=count)
    assert len([g for g in enf.groups if g]) == (1 if count <= 64 else 3)
    labels = random_labels(rng, enf.names, n)
    total, full = enf.enforce(labels)
    assert len(full) == n
    want = {k: b for k, b in full.items() if b != b"[]"}
    assert 0 < len(want)
    got_total, got = enf.enforce_changes(labels)
    assert got_total == total and got == want
    assert list(got) == [x for x in nodes if x in want]  # ascending node order
    # skip_settled: fewer or shorter bodies, the same labels afterwards
    red_total, reduced = enf.enforce_changes(labels, skip_settled=True)
    assert red_total == total and set(reduced) <= set(want)
    assert sum(map(len, reduced.values())) < sum(map(len, want.values()))
    patched = []
    for i, name in enumerate(nodes):
        after_full = apply_label_patch(labels[i], full[name])
        after_reduced = apply_label_patch(labels[i], reduced.get(name, b"[]"))
        assert after_full == after_reduced, name
        patched.append(after_full)
    assert enf.enforce_changes(patched, skip_settled=True) == (total, {})
    # (without skip_settled a settled cluster is patched again on every pass)
    assert len(enf.enforce_changes(patched)[1]) > 0


def test_enforce_changes_no_strategies(ctx):
    enf, nodes, rng = enforcer_case(ctx, 8390, 10, [], seed=1)
    assert enf.enforce_changes([{} for _ in nodes]) == (0, {})
    assert enf.enforce([{} for _ in nodes])[0] == 0
