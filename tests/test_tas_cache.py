"""TasCache (pas_amd/tas_cache.py) and MetricsExtender.snapshot_changed.

The checker of the GPU part is a dict model of AutoUpdatingCache written here: cache =
{name: map-or-None} as the actor holds it (cache.go:43-63) and metricMap = {name: int}
(autoupdating.go:105-137).  After every step arrays are built from the model from scratch over
the cache's current node_names / metric_names, pas_tas_snapshot_get is compared with them,
and one filter + prioritize batch and one deschedule sweep are compared with the oracle's
per-value decimal form.

The CPU part needs no GPU: the order in which one refresh plans its device calls (against a
recording context), the slots= mode, and the extender's tables."""
from decimal import Decimal

import numpy as np
import pytest

from pas_amd import extender, snapshot
from pas_amd.tas_cache import TasCache
from pas_amd.workload import pack_bits, unpack_bits
from helpers import RULE_DTYPE

WIDE_VALUES = ["10000000000000000", "0.0000001", "1000000000000", "3", "7.5"]


class Model:
    """AutoUpdatingCache's metric half, as the reference holds it."""

    def __init__(self):
        self.cache = {}
        self.metric_map = {}

    def write(self, name, data):  # WriteMetric + the actor's WRITE
        payload = dict(data) if data else None
        if payload is None:
            payload = self.cache.get(name)
            self.metric_map[name] = self.metric_map[name] + 1 if name in self.metric_map else 1
        self.cache[name] = payload

    def delete(self, name):  # DeleteMetric
        if name in self.metric_map and self.metric_map[name] == 1:
            del self.metric_map[name]
            self.cache.pop(name, None)
        else:
            self.metric_map[name] = self.metric_map.get(name, 0) - 1

    def update_all(self, fetch):  # updateAllMetrics
        for name in list(self.metric_map):
            if name == "":
                del self.metric_map[name]
                continue
            try:
                result = fetch(name)
            except Exception:
                continue
            self.write(name, result)

    def held(self):
        return {name for name, data in self.cache.items() if data}


def oracle_arrays(model, node_names, metric_names):
    """Per-value (u, s): value = u * 10^-s at the value's own decimal places; presence."""
    m, n = len(metric_names), len(node_names)
    u = np.zeros((m, n), np.int64)
    s = np.zeros((m, n), np.int8)
    pres = np.zeros((m, n), bool)
    index = {name: i for i, name in enumerate(node_names) if name is not None}
    for c, name in enumerate(metric_names):
        held = (model.cache.get(name) or {}) if name is not None else {}
        for node, q in held.items():
            d = Decimal(q)
            places = max(0, -d.as_tuple().exponent)
            u[c, index[node]], s[c, index[node]] = int(d.scaleb(places)), places
            pres[c, index[node]] = True
    return u, s, pres


def check(ctx, oracle, tc, model):
    assert set(tc.metric_index) == model.held()
    assert all(tc.metric_names[c] == name for name, c in tc.metric_index.items())
    assert sum(name is not None for name in tc.metric_names) == len(tc.metric_index)
    n, m = len(tc.node_names), len(tc.metric_names)
    assert all(tc.node_names[i] == name for name, i in tc.node_index.items())
    # from scratch, as a cold start would encode the model
    metrics = {name: model.cache[name] for name in tc.metric_index}
    cols = [name if name is not None else "" for name in tc.metric_names]
    v, p, scale, wide = snapshot.tas_snapshot_from_metrics_wide(metrics, tc.node_names, cols)
    gen, vals, present, gscale, gwide, nano = ctx.tas_snapshot_get()
    assert gen == tc.gen and vals.shape == (m, n)
    np.testing.assert_array_equal(present, p)
    pres = unpack_bits(present, n)
    assert [int(x) for x in gwide] == [int(c in wide) for c in range(m)]
    for c in range(m):
        want_v, want_f = (wide[c] if c in wide else (v[c], np.zeros(n, np.uint32)))
        np.testing.assert_array_equal(np.where(pres[c], vals[c], 0), np.where(pres[c], want_v, 0))
        np.testing.assert_array_equal(np.where(pres[c], nano[c], 0), np.where(pres[c], want_f, 0))
        if c not in wide:  # (a wide column keeps the scale recorded before it became wide)
            assert gscale[c] == scale[c], (c, tc.metric_names[c])
    # one batch and one sweep against the oracle
    u, s, opres = oracle_arrays(model, tc.node_names, tc.metric_names)
    np.testing.assert_array_equal(opres, pres)
    targets = [5, 10, 10**12]
    rules = np.array([(c, c % 3, targets[(c // 3) % 3]) for c in range(m)] + [(-1, 0, 0)],
                     RULE_DTYPE)
    off = np.arange(len(rules) + 1, dtype=np.int32)
    prio = np.array([(c % m, (c + 1) % 3, 0) for c in range(len(rules))], RULE_DTYPE)
    gp, go, gl = ctx.tas_eval(tc.gen, rules, off, prio)
    wp, wo, wl = oracle.tas_eval(u, pack_bits(opres), rules, off, prio, v_scale=s)
    np.testing.assert_array_equal(gp, wp)
    np.testing.assert_array_equal(gl, wl)
    for i in range(len(gl)):
        np.testing.assert_array_equal(go[i, :gl[i]], wo[i, :wl[i]])
    np.testing.assert_array_equal(ctx.tas_violations(tc.gen, rules, off),
                                  oracle.tas_violations(u, pack_bits(opres), rules, off,
                                                        v_scale=s))


def drive(ctx, oracle, seed, n_steps=60):
    rng = np.random.default_rng(seed)
    nodes = [f"n{i:02d}" for i in range(40)]
    seen = {"new_nodes": 0}

    def quantity():
        k = int(rng.integers(0, 5))
        whole = int(rng.integers(0, 20))
        return [str(whole), f"{whole}.5", f"{whole}.25", f"{whole}.000125", str(whole * 1000)][k]

    def node_map(frac=0.7, grow=0):
        for _ in range(grow):
            nodes.append(f"x{seen['new_nodes']:03d}")
            seen["new_nodes"] += 1
        keep = [n for n in nodes if rng.random() < frac]
        return {n: quantity() for n in keep}

    def wide_map():
        mp = {n: str(rng.choice(WIDE_VALUES)) for n in nodes if rng.random() < 0.7}
        mp[nodes[0]], mp[nodes[1]] = WIDE_VALUES[1], WIDE_VALUES[2]  # wide is needed
        return mp

    model = Model()
    start = {"a": node_map(), "b": node_map()}
    for name, mp in start.items():
        model.write(name, mp)
    tc = TasCache.from_metrics(ctx, 880000 + 10000 * seed, start, node_names=nodes)
    assert (len(tc.node_names), len(tc.metric_names)) == (40, 2)
    check(ctx, oracle, tc, model)

    policies, pool = [], [f"m{i}" for i in range(9)] + ["a", "b"]
    freed, stats = set(), dict(node_growth=0, col_growth=0, wide_carried=0, reuse=0,
                               del_unregistered=0, raised=0, empty=0)

    def both(fn_name, *args):
        getattr(model, {"write_metric": "write", "delete_metric": "delete",
                        "update_all_metrics": "update_all"}[fn_name])(*args)
        getattr(tc, fn_name)(*args)

    def refresh(grow=0, clean=False):
        results = {}
        for name in list(model.metric_map):
            kind = 1.0 if clean else rng.random()
            if kind < 0.1:
                results[name] = RuntimeError("metrics API")
                stats["raised"] += 1
            elif kind < 0.2:
                results[name] = {}
                stats["empty"] += 1
            elif name == "w":
                results[name] = wide_map()
            else:  # nodes come (grow) and go (frac)
                results[name] = node_map(frac=float(rng.choice([0.4, 0.7, 1.0])), grow=grow)
                grow = 0

        def fetch(name):
            if isinstance(results[name], Exception):
                raise results[name]
            return results[name]
        both("update_all_metrics", fetch)

    def add_policy(names=None):
        names = names or [str(x) for x in rng.choice(pool, size=int(rng.integers(1, 4)),
                                                     replace=False)]
        policies.append(names)
        for name in names:
            both("write_metric", name, None)

    def delete_policy(i):
        for name in policies.pop(i):
            both("delete_metric", name)

    # the scripted steps every sequence contains, among the drawn ones (clean: every name
    # gets data, none raises)
    script = {0: lambda: both("write_metric", "w", wide_map()),   # data, no registration
              1: lambda: add_policy(["a", "m0"]),
              2: lambda: refresh(grow=3, clean=True),             # m0's first data, new nodes
              20: lambda: add_policy(["z1"]),
              21: lambda: refresh(clean=True),
              22: lambda: delete_policy(len(policies) - 1),       # count 1: column freed
              23: lambda: add_policy(["z2"]),
              24: lambda: refresh(grow=70, clean=True),           # reuse; more than 64 new nodes
              25: lambda: both("delete_metric", "never-registered")}
    for step in range(n_steps):
        shape = (len(tc.node_names), len(tc.metric_names))
        wide_before = {tc.metric_names[c] for c in range(shape[1]) if tc.wide[c]}
        cols_before = dict(tc.metric_index)
        counts_before = dict(model.metric_map)
        if step in script:
            script[step]()
        else:
            what = str(rng.choice(["add", "delete", "refresh", "refresh", "grow", "write",
                                   "stray"]))
            if what == "add" or (what == "delete" and not policies):
                add_policy()
            elif what == "delete":
                delete_policy(int(rng.integers(len(policies))))
            elif what == "refresh":
                refresh()
            elif what == "grow":
                refresh(grow=int(rng.integers(1, 4)))
            elif what == "write":
                both("write_metric", str(rng.choice(pool)), node_map())
            else:
                both("delete_metric", f"stray{step}")
        for name in set(model.metric_map) - set(counts_before):
            if model.metric_map[name] == -1:
                stats["del_unregistered"] += 1
        now = (len(tc.node_names), len(tc.metric_names))
        if now != shape:
            stats["node_growth"] += now[0] != shape[0]
            stats["col_growth"] += now[1] != shape[1]
            stats["wide_carried"] += any(tc.wide[tc.metric_index[name]] for name in wide_before
                                         if name in tc.metric_index)
        freed |= {c for name, c in cols_before.items() if name not in tc.metric_index}
        for name, c in tc.metric_index.items():
            if name not in cols_before and c in freed:
                stats["reuse"] += 1
                freed.discard(c)
        check(ctx, oracle, tc, model)
    return tc, model, stats


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sequences_match_the_model(ctx, oracle, seed):
    tc, model, stats = drive(ctx, oracle, seed)
    assert stats["node_growth"] >= 1 and stats["col_growth"] >= 1, stats
    assert stats["wide_carried"] >= 1 and stats["reuse"] >= 1, stats
    assert stats["del_unregistered"] >= 1, stats
    assert "w" in tc.metric_index and "w" not in model.metric_map  # written, never refreshed
    assert len(tc.node_names) > 40 + 64 and len(tc.metric_names) >= 10


@pytest.mark.gpu
def test_reference_quirks(ctx, oracle):
    model = Model()
    start = {"a": {"n0": "1", "n1": "2.5"}}
    model.write("a", start["a"])
    tc = TasCache.from_metrics(ctx, 870000, start, spare_nodes=2, spare_metrics=1)
    asked = []

    def fetch_for(results):
        def fetch(name):
            asked.append(name)
            return results.get(name, {})
        return fetch

    def both(fn_name, *args):
        getattr(model, {"write_metric": "write", "delete_metric": "delete",
                        "update_all_metrics": "update_all"}[fn_name])(*args)
        getattr(tc, fn_name)(*args)
        assert tc.counts == model.metric_map
        check(ctx, oracle, tc, model)

    # count -1 -> register -> 0 -> delete -> -1: still registered, still refreshed
    both("delete_metric", "q")
    assert tc.counts["q"] == -1
    both("write_metric", "q", None)
    assert tc.counts["q"] == 0
    both("delete_metric", "q")
    assert tc.counts["q"] == -1
    asked.clear()
    both("update_all_metrics", fetch_for({"q": {"n1": "4", "n2": "0.5"}}))
    assert set(asked) == {"q"} and tc.metric_index["q"] == 1 and tc.node_index["n2"] == 2
    # an unregistered name written with data ("a") was not asked for; an empty fetch bumps
    asked.clear()
    both("update_all_metrics", fetch_for({}))
    assert set(asked) == {"q"} and tc.counts["q"] == 0 and "q" in tc.metric_index
    both("update_all_metrics", fetch_for({}))
    assert tc.counts["q"] == 1
    gen = tc.gen
    both("delete_metric", "q")  # exactly 1: registration and data go, the column is free
    assert "q" not in tc.counts and tc.metric_names == ["a", None] and tc.gen == gen + 1
    both("write_metric", "r", {"n3": "9"})  # reuses the column and the last spare slot
    assert tc.metric_index["r"] == 1 and tc.node_names == ["n0", "n1", "n2", "n3"]
    both("write_metric", "", None)  # the empty name is unregistered by the next refresh
    both("update_all_metrics", fetch_for({}))
    assert "" not in tc.counts


# ------------------------------------------------------------------ CPU: planning

class RecordingCtx:
    """Records the device calls TasCache plans, in order."""

    def __init__(self):
        self.calls = []

    def tas_snapshot_reshape(self, gen_from, gen_to, n_nodes, n_metrics, src_col=None,
                             stream=None):
        self.calls.append(("reshape", gen_from, gen_to, n_nodes, n_metrics, src_col))

    def tas_snapshot_update(self, gen_from, gen_to, cols, v, p):
        self.calls.append(("update", gen_from, gen_to, list(cols), np.asarray(v).shape))

    def tas_snapshot_update_wide(self, gen_from, gen_to, cols, whole, nano, p):
        self.calls.append(("update_wide", gen_from, gen_to, list(cols),
                           np.asarray(whole).shape))

    def tas_snapshot_set_scale(self, gen, scale, stream=None):
        self.calls.append(("set_scale", gen, [int(s) for s in scale]))


def fetch_from(results):
    return lambda name: results[name]


def test_one_refresh_plans_each_call_once():
    ctx = RecordingCtx()
    tc = TasCache(ctx, 100, ["a", "b"], ["m0"])
    tc.data["m0"] = {"a": "1"}
    for name in ("m0", "m1", "mw"):
        tc.write_metric(name)
    assert ctx.calls == [] and tc.counts == {"m0": 1, "m1": 1, "mw": 1}
    assert tc.metric_index == {"m0": 0}  # registered names without data own no column
    tc.update_all_metrics(fetch_from({
        "m0": {"a": "1.000001", "b": "2", "c": "3"},        # a new node, six decimal places
        "m1": {"a": "5"},                                    # first data: a new column
        "mw": {"a": "0.0000001", "b": "1000000000000"}}))    # only a wide column holds both
    assert ctx.calls == [
        ("reshape", 100, 101, 66, 9, None),
        ("update", 101, 102, [0, 1], (2, 66)),
        ("update_wide", 102, 103, [2], (1, 66)),
        ("set_scale", 103, [6] + [3] * 8)]
    assert tc.gen == 103 and tc.node_index["c"] == 2 and tc.node_names[3:] == [None] * 63
    assert tc.metric_names == ["m0", "m1", "mw"] + [None] * 6
    assert tc.wide[:3] == [False, False, True]


def test_a_refresh_with_room_plans_no_reshape():
    ctx = RecordingCtx()
    tc = TasCache(ctx, 7, ["a", None], ["m0", None])
    tc.write_metric("m0")
    tc.write_metric("m1")
    tc.update_all_metrics(fetch_from({"m0": {"a": "1", "c": "2"}, "m1": {"c": "4"}}))
    assert ctx.calls == [("update", 7, 8, [0, 1], (2, 2))]
    assert tc.node_names == ["a", "c"] and tc.metric_names == ["m0", "m1"] and tc.gen == 8
    # an empty result and a raise plan nothing; the empty one bumps the count
    def fetch(name):
        if name == "m0":
            raise RuntimeError("metrics API")
        return {}
    tc.update_all_metrics(fetch)
    assert len(ctx.calls) == 1 and tc.counts == {"m0": 1, "m1": 2}
    # the last user's delete empties the column
    tc.delete_metric("m0")
    assert ctx.calls[1] == ("update", 8, 9, [0], (1, 2)) and tc.metric_names == [None, "m1"]


class Slots:
    def __init__(self, names):
        self.node_names = names
        self.node_index = {n: i for i, n in enumerate(names) if n is not None}


def test_slots_are_followed_not_picked():
    ctx = RecordingCtx()
    slots = Slots(["a", "b", None])
    tc = TasCache(ctx, 1, ["a", "b"], ["m0"], slots=slots)
    tc.write_metric("m0", {"a": "1", "b": "2", "zz": "3"})
    assert tc.skipped_nodes == {"zz"} and slots.node_names == ["a", "b", None]
    assert tc.node_names == ["a", "b", None] and "zz" not in tc.node_index
    assert ctx.calls == [("reshape", 1, 2, 3, 1, None), ("update", 2, 3, [0], (1, 3))]
    # the name gets its slot from the owner of the slots; the next write installs it
    slots.node_names[2] = "zz"
    slots.node_index["zz"] = 2
    tc.write_metric("m0", {"zz": "3"})
    assert tc.skipped_nodes == set() and tc.node_index["zz"] == 2
    assert ctx.calls[2:] == [("update", 3, 4, [0], (1, 3))]


def test_extender_tables_follow_the_cache():
    ext = extender.MetricsExtender(None, 1, ["a", "b"], ["m0"], {})
    ext.snapshot_changed(5, ["a", None, "c"], ["m0", None, "m2"])
    assert ext.gen == 5 and ext.node_names == ["a", "", "c"]
    assert ext.node_index == {"a": 0, "c": 2} and ext.metric_index == {"m0": 0, "m2": 2}
    assert len(ext._rules([("m2", "LessThan", 1), ("gone", "LessThan", 1)])) == 2
    assert list(ext._rules([("m2", "LessThan", 1), ("gone", "LessThan", 1)])["metric"]) == [2, -1]
