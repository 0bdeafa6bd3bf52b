"""PolicyCache (pas_amd/policy_cache.py) against a restatement, written here, of the
reference's TelemetryPolicyController events (controller/controller.go:61-176) and its
MetricEnforcer registry (strategies/core/enforcer.go:64-103), over a recording context: no GPU.

After every scripted event the metric registrations, the policy ids, the table handed to
pas_tas_policies_set and the deschedule strategy list are compared with the model's."""
import numpy as np

from pas_amd import _lib
from pas_amd.extender import DescheduleEnforcer
from pas_amd.policy_cache import PolicyCache, TasPolicy
from pas_amd.tas_cache import TasCache
from helpers import OPS, RULE_DTYPE

TYPES = ("scheduleonmetric", "deschedule", "dontschedule")
NEW = ("pas_tas_policies_set", "pas_tas_policies_info", "pas_tas_policies_drop",
       "pas_tas_policies_violated", "pas_tas_policies_violated_device", "pas_tas_eval_policies",
       "pas_tas_eval_policies_device", "pas_tas_filter_requests_policies",
       "pas_tas_filter_requests_policies_device")


def test_lib_declares_the_new_functions():
    for name in NEW:
        assert name in _lib.SIGNATURES, name


# ------------------------------------------------------------------------- the model

def spec_of(spec):
    """(PolicyName field, Rules) of a TASPolicyStrategy; the zero value for a missing one."""
    if spec is None:
        return "", []
    if isinstance(spec, dict):
        return spec.get("policyName", ""), list(spec["rules"])
    return "", list(spec)


def equals(a, b):  # deschedule/strategy.go:60-78
    return (a[0] == b[0] and len(a[1]) > 0 and len(a[1]) == len(b[1])
            and all(x == y for x, y in zip(a[1], b[1])))


class Model:
    """The controller, the cache's policy half, metricMap and the enforcer's deschedule set."""

    def __init__(self):
        self.policies = {}     # "policies/<ns>/<name>"
        self.registry = []     # RegisteredStrategies["deschedule"], registration order
        self.metric_map = {}   # AutoUpdatingCache.metricMap
        self.calls = []        # WriteMetric(name, nil) / DeleteMetric(name), in order

    def write_metric(self, name):  # autoupdating.go:105-116, nil payload
        self.calls.append(("write", name))
        self.metric_map[name] = self.metric_map[name] + 1 if name in self.metric_map else 1

    def delete_metric(self, name):  # :127-137
        self.calls.append(("delete", name))
        if self.metric_map.get(name) == 1:
            del self.metric_map[name]
        else:
            self.metric_map[name] = self.metric_map.get(name, 0) - 1

    def add_strategy(self, stype, strategy):  # enforcer.go:84-103
        if stype != "deschedule":  # the other types are not Enforceable: nothing is stored
            return
        if any(equals(s, strategy) for s in self.registry):
            return
        self.registry.append(strategy)

    def remove_strategy(self, stype, strategy):  # :64-82 (Cleanup is out of scope)
        if stype == "deschedule":
            self.registry = [s for s in self.registry if not equals(s, strategy)]

    def on_add(self, pol):  # controller.go:61-91
        self.policies[(pol.namespace, pol.name)] = pol
        for stype, spec in pol.strategies.items():
            if stype not in TYPES:
                return
            _, rules = spec_of(spec)
            self.add_strategy(stype, (pol.name, rules))  # SetPolicyName(ObjectMeta.Name)
            for rule in rules:
                self.write_metric(rule[0])

    def on_update(self, old, new):  # :111-149
        self.policies[(new.namespace, new.name)] = new
        for stype, spec in new.strategies.items():
            if stype not in TYPES:
                return
            old_strategy = spec_of(old.strategies.get(stype))  # no SetPolicyName here
            self.remove_strategy(stype, old_strategy)
            for rule in old_strategy[1]:
                self.delete_metric(rule[0])
            _, rules = spec_of(spec)
            self.add_strategy(stype, (new.name, rules))
            for rule in rules:
                self.write_metric(rule[0])

    def on_delete(self, pol):  # :152-176
        for stype, spec in pol.strategies.items():
            if stype not in TYPES:
                return
            _, rules = spec_of(spec)
            self.remove_strategy(stype, (pol.name, rules))
            for rule in rules:
                self.delete_metric(rule[0])
        self.policies.pop((pol.namespace, pol.name), None)


def expected_table(model, ids, metric_index):
    """Row i of the table: the dontschedule rules and scheduleonmetric Rules[0] of the policy
    with id i, names resolved to columns; an id nobody holds is an empty row."""
    n = max(ids.values(), default=-1) + 1
    by_id = {i: key for key, i in ids.items()}
    rules, off, prio = [], [0], []
    for i in range(n):
        pol = model.policies.get(by_id.get(i))
        strategies = {t: spec_of(s)[1] for t, s in pol.strategies.items()} if pol else {}
        for m, o, t in strategies.get("dontschedule", []):
            rules.append((metric_index.get(m, -1), OPS.get(o, 3), t))
        off.append(len(rules))
        p = strategies.get("scheduleonmetric", [])
        if p and p[0][0] and p[0][0] in metric_index:
            prio.append((metric_index[p[0][0]], OPS.get(p[0][1], 3), p[0][2]))
        else:
            prio.append((-1, 0, 0))
    return (np.array(rules, RULE_DTYPE), np.array(off, np.int32), np.array(prio, RULE_DTYPE))


# ------------------------------------------------------------------------- the fakes

class RecordingCtx:
    """Records the table of every pas_tas_policies_set (and the metric half's device calls)."""

    def __init__(self):
        self.tables = []
        self.other = []

    def tas_policies_set(self, rules, rule_off, prio):
        self.tables.append((np.array(rules, RULE_DTYPE), np.array(rule_off, np.int32),
                            np.array(prio, RULE_DTYPE)))

    def tas_snapshot_update(self, gen_from, gen_to, cols, v, p):
        self.other.append(("update", list(cols)))

    def tas_snapshot_set_scale(self, gen, scale, stream=None):
        self.other.append(("set_scale",))


class RecordingMetrics:
    """The metric half as PolicyCache sees it: the calls, and fixed columns."""

    def __init__(self, metric_index):
        self.metric_index = dict(metric_index)
        self.calls = []

    def write_metric(self, name, data=None):
        assert data is None
        self.calls.append(("write", name))

    def delete_metric(self, name):
        self.calls.append(("delete", name))


# ------------------------------------------------------------------------- the script

COLUMNS = {"cpu": 0, "mem": 1, "temp": 3}  # "power" and "" have no column

A1 = TasPolicy("ns1", "pol-a", {
    "dontschedule": [("cpu", "GreaterThan", 80), ("mem", "LessThan", 10)],
    "scheduleonmetric": [("cpu", "LessThan", 0)],
    "deschedule": [("temp", "GreaterThan", 90)]})
# the same name in another namespace: SetPolicyName drops the namespace, so its deschedule
# strategy Equals A1's and is not added; its prio metric has no column
B = TasPolicy("ns2", "pol-a", {
    "deschedule": [("temp", "GreaterThan", 90)],
    "dontschedule": [("power", "Equals", 5), ("temp", "NotAnOperator", 1)],
    "scheduleonmetric": [("power", "GreaterThan", 0)]})
# an invalid strategy type between two valid ones: the loop returns there
C = TasPolicy("ns1", "pol-c", {
    "dontschedule": [("mem", "GreaterThan", 7)],
    "labeling": [("cpu", "GreaterThan", 1)],
    "deschedule": [("cpu", "GreaterThan", 99)]})
# A without its scheduleonmetric strategy (a type only in the old policy) and others changed
A2 = TasPolicy("ns1", "pol-a", {
    "dontschedule": [("cpu", "GreaterThan", 85)],
    "deschedule": [("temp", "GreaterThan", 95), ("cpu", "LessThan", 1)]})
# ... and with one again (a type only in the new policy)
A3 = TasPolicy("ns1", "pol-a", {
    "scheduleonmetric": [("mem", "GreaterThan", 0), ("cpu", "LessThan", 0)],
    "dontschedule": [("cpu", "GreaterThan", 85)],
    "deschedule": [("temp", "GreaterThan", 95), ("cpu", "LessThan", 1)]})
# the object's own PolicyName field says the object's name: onUpdate finds the old strategy
D1 = TasPolicy("ns1", "pol-d", {
    "deschedule": {"policyName": "pol-d", "rules": [("mem", "LessThan", 3)]}})
D2 = TasPolicy("ns1", "pol-d", {
    "deschedule": {"policyName": "pol-d", "rules": [("mem", "LessThan", 4)]},
    "scheduleonmetric": [("", "LessThan", 0)]})
E = TasPolicy("ns3", "pol-e", {"dontschedule": [("temp", "Equals", 1)]})

SCRIPT = [("add", A1), ("add", B), ("add", C), ("update", A1, A2), ("update", A2, A3),
          ("add", D1), ("update", D1, D2), ("delete", B), ("delete", C), ("add", E),
          ("delete", A3), ("delete", D2), ("delete", E)]


def apply(target, step):
    getattr(target, "on_" + step[0])(*step[1:])


def assert_table(got, want):
    for g, w, what in zip(got, want, ("rules", "rule_off", "prio")):
        np.testing.assert_array_equal(g, w, err_msg=what)


def test_events_against_the_restatement():
    ctx, metrics, model = RecordingCtx(), RecordingMetrics(COLUMNS), Model()
    cache = PolicyCache(ctx, metrics)
    assert len(ctx.tables) == 1 and len(ctx.tables[0][1]) == 1  # the empty table
    want_ids = {}
    for k, step in enumerate(SCRIPT):
        apply(cache, step)
        apply(model, step)
        # stable ids: a policy keeps its id; a new one takes the lowest free id
        for key in model.policies:
            if key not in want_ids:
                want_ids[key] = min(set(range(len(want_ids) + 1)) - set(want_ids.values()))
        for key in [key for key in want_ids if key not in model.policies]:
            del want_ids[key]
        what = f"step {k} ({step[0]} {step[-1].namespace}/{step[-1].name})"
        assert cache.ids == want_ids, what
        assert set(cache.policies) == set(model.policies), what
        assert metrics.calls == model.calls, what
        assert cache.strategies == model.registry, what
        assert len(ctx.tables) == k + 2, f"{what}: one pas_tas_policies_set per event"
        want = expected_table(model, want_ids, COLUMNS)
        assert_table(ctx.tables[-1], want)
        for key, i in want_ids.items():
            assert tuple(cache.prio_of(i)) == tuple(want[2][i]), what
            assert cache.id_of(key) == i
    # what the script has met on its way
    assert model.registry == [] and model.calls.count(("delete", "temp")) >= 2
    assert ("ns1", "pol-c") in model.policies  # onDelete returned before DeletePolicy


def test_the_quirks_the_script_relies_on():
    ctx, metrics = RecordingCtx(), RecordingMetrics(COLUMNS)
    cache = PolicyCache(ctx, metrics)
    cache.on_add(A1)
    cache.on_add(B)
    assert cache.strategies == [("pol-a", [("temp", "GreaterThan", 90)])]  # B's is a duplicate
    assert cache.ids == {("ns1", "pol-a"): 0, ("ns2", "pol-a"): 1}
    rules, off, prio = ctx.tables[-1]
    assert list(off) == [0, 2, 4]
    assert [tuple(r) for r in rules] == [(0, 1, 80), (1, 0, 10), (-1, 2, 5), (3, 3, 1)]
    assert [tuple(p) for p in prio] == [(0, 0, 0), (-1, 0, 0)]
    cache.on_add(C)
    # the invalid type ended the event: C is written, its deschedule strategy is not registered
    assert len(cache.strategies) == 1 and ("ns1", "pol-c") in cache.policies
    assert metrics.calls[-1] == ("write", "mem")
    n = len(metrics.calls)
    cache.on_update(A1, A2)
    # the old strategy carries no policy name, so it is not found and stays registered; the
    # old scheduleonmetric strategy's metric stays registered (its type is not walked)
    assert [s[0] for s in cache.strategies] == ["pol-a", "pol-a"]
    assert metrics.calls[n:] == [("delete", "cpu"), ("delete", "mem"), ("write", "cpu"),
                                 ("delete", "temp"), ("write", "temp"), ("write", "cpu")]
    cache.on_add(D1)
    cache.on_update(D1, D2)
    assert [s for s in cache.strategies if s[0] == "pol-d"] == [("pol-d", [("mem", "LessThan", 4)])]
    assert tuple(cache.prio_of(cache.id_of(("ns1", "pol-d")))) == (-1, 0, 0)  # no metric name
    assert cache.get(("ns1", "pol-d"))["deschedule"] == [("mem", "LessThan", 4)]
    assert cache.get(("nowhere", "pol-d")) is None
    assert cache.read_policy("ns1", "pol-d") is D2
    cache.on_delete(B)
    assert ("ns2", "pol-a") not in cache.ids and list(ctx.tables[-1][1][:3]) == [0, 1, 1]
    cache.on_add(E)
    assert cache.id_of(("ns3", "pol-e")) == 1  # the freed id


def test_registration_counts_through_a_tas_cache():
    # the same script over a real TasCache (on the recording context): metricMap follows
    ctx, model = RecordingCtx(), Model()
    tc = TasCache(ctx, 1, ["n0", "n1"], ["cpu", "mem", None, "temp"])
    cache = PolicyCache(ctx, tc)
    for step in SCRIPT[:8]:
        apply(cache, step)
        apply(model, step)
        assert tc.counts == model.metric_map, step[0]
    assert model.metric_map["temp"] >= 1 and model.metric_map["cpu"] >= 2
    for step in SCRIPT[8:]:
        apply(cache, step)
        apply(model, step)
        assert tc.counts == model.metric_map, step[0]


def test_snapshot_changed_resolves_the_names_again():
    ctx = RecordingCtx()
    cache = PolicyCache(ctx, metric_names=["cpu", "mem", None, "temp"])
    cache.on_add(A1)
    assert [int(m) for m in ctx.tables[-1][0]["metric"]] == [0, 1]
    cache.snapshot_changed(7, ["n0"], ["mem", None, "cpu"])
    assert len(ctx.tables) == 3
    assert [int(m) for m in ctx.tables[-1][0]["metric"]] == [2, 0]
    assert tuple(cache.prio_of(0)) == (2, 0, 0)
    cache.snapshot_changed(8, ["n0"], ["mem"])
    assert [int(m) for m in ctx.tables[-1][0]["metric"]] == [-1, 0]
    assert tuple(cache.prio_of(0)) == (-1, 0, 0)


def test_strategies_feed_the_deschedule_enforcer():
    # the registry is the `strategies` list DescheduleEnforcer takes (no device call here)
    ctx = RecordingCtx()
    cache = PolicyCache(ctx, metric_names=["cpu", "mem", None, "temp"])
    for pol in (A1, B, D1):
        cache.on_add(pol)
    enf = DescheduleEnforcer(ctx, 1, ["n0", "n1"], ["cpu", "mem", None, "temp"],
                             cache.strategies)
    assert enf.names == ["pol-a", "pol-d"]
    assert [tuple(r) for r in enf.rules] == [(3, 1, 90), (1, 0, 3)]
    assert list(enf.rule_off) == [0, 1, 2]
