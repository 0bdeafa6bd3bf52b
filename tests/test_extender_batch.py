"""MetricsExtender.filter_batch / prioritize_batch and GASExtender.filter_batch: a micro-batch
of concurrent requests answered through one *_requests call each must be byte-equal to the
single verbs called one by one, every early return and the tie order included.  Bodies modelled
on tests/test_extender.py."""
import json

import pytest

from pas_amd import extender as ext
from pas_amd import snapshot as sn
from test_extender import args, gas_pod

pytestmark = pytest.mark.gpu

NODES = [f"node-{i:02d}" for i in range(40)]
POLICIES = {
    ("default", "test-policy"): {
        "scheduleonmetric": [("dummyMetric1", "GreaterThan", 0)],
        "dontschedule": [("dummyMetric1", "GreaterThan", 10)]},
    ("default", "less"): {
        "scheduleonmetric": [("dummyMetric1", "LessThan", 0)],
        "dontschedule": [("dummyMetric1", "LessThan", 10), ("absentMetric", "Foo", 1),
                         ("emptyMetric", "Bar", 2), ("second", "Equals", 7)]},
    ("default", "only-sched"): {"scheduleonmetric": [("second", "GreaterThan", 0)]},
    ("default", "only-dont"): {"dontschedule": [("second", "GreaterThan", 3)]},
    ("default", "not-cached"): {"scheduleonmetric": [("absentMetric", "GreaterThan", 0)],
                                "dontschedule": [("absentMetric", "GreaterThan", 0)]},
    ("default", "odd-operator"): {"scheduleonmetric": [("dummyMetric1", "Foo", 0)]},
    ("default", "panics"): {"dontschedule": [("second", "LessThan", 1),
                                             ("dummyMetric1", "Foo", 1)]},
}


def lab(policy):
    return {"telemetry-policy": policy}


def tas(ctx, gen):
    # three values over forty nodes, so ties dominate; a few nodes without either metric
    m1 = {n: str(10 * (i % 3)) for i, n in enumerate(NODES) if i % 11 != 5}
    m2 = {n: str(i % 8) for i, n in enumerate(NODES) if i % 7 != 3}
    metrics = ["dummyMetric1", "second", "emptyMetric"]
    v, pres, scale = sn.tas_snapshot_from_metrics(
        {"dummyMetric1": m1, "second": m2, "emptyMetric": {}}, NODES, metrics)
    ctx.tas_snapshot_set(gen, v, pres, scale)
    return ext.MetricsExtender(ctx, gen, NODES, metrics, POLICIES)


def tas_bodies():
    rev = NODES[::-1]
    return [
        b"",                                                      # decode error
        b"{}",                                                    # Nodes == nil
        args({"useless-label": "x"}, NODES[:5]),                  # no policy label
        args(lab("nowhere"), NODES[:5]),                          # policy not found
        args(lab("test-policy"), NODES),                          # snapshot order
        args(lab("test-policy"), rev),                            # reverse order, tied values
        args(lab("test-policy"), []),                             # no nodes
        args(lab("less"), NODES[3:30:2] + ["ghost-1", "ghost-2"] + NODES[:3]),  # unknown names
        args(lab("test-policy"), [NODES[7], NODES[2], NODES[7], NODES[2], NODES[8]]),  # repeats
        args(lab("only-sched"), rev[5:25], key_case=str.lower),   # no dontschedule rules
        args(lab("only-dont"), NODES[10:]),                       # no scheduleonmetric rule
        args(lab("not-cached"), NODES[:9]),                       # metric not cached
        args(lab("odd-operator"), rev[:12]),                      # unsorted list / no rules
        args(lab("less"), ["ghost-1"]),                           # only unknown names
    ]


def test_tas_filter_batch_is_byte_equal_to_the_single_verb(ctx):
    m = tas(ctx, 8600)
    bodies = tas_bodies()
    want = [m.filter(b) for b in bodies]
    assert m.filter_batch(bodies) == want
    # every kind of answer is in the batch
    assert {w[0] for w in want} == {200, 404}
    assert (200, b"") in want and (404, b"null\n") in want
    full = [json.loads(w[1]) for w in want if w[0] == 200 and w[1]]
    assert any(r["FailedNodes"] for r in full) and any("ghost-1" in (r["NodeNames"] or [])
                                                       for r in full)
    assert m.filter_batch([]) == []
    assert m.filter_batch(bodies[:4]) == want[:4]  # nothing left for the library


def test_tas_prioritize_batch_is_byte_equal_to_the_single_verb(ctx):
    m = tas(ctx, 8601)
    bodies = tas_bodies() + [args({"useless-label": "x"}, [])]
    want = [m.prioritize(b) for b in bodies]
    assert m.prioritize_batch(bodies) == want
    assert {w[0] for w in want} == {200, 400}
    assert (200, b"") in want and (200, b"[]\n") in want and (400, b"[]\n") in want
    # the reverse-order request: its ties follow the request, not the snapshot's numbering
    # (where the old micro-batch route through pas_tas_eval would differ)
    fwd = [h["Host"] for h in json.loads(want[4][1])]
    rev = [h["Host"] for h in json.loads(want[5][1])]
    assert sorted(fwd) == sorted(rev) and fwd != rev
    top = [n for i, n in enumerate(NODES) if i % 3 == 2 and i % 11 != 5]
    assert fwd[: len(top)] == top and rev[: len(top)] == top[::-1]
    assert m.prioritize_batch([]) == []


def test_tas_filter_batch_panics_as_the_single_verb(ctx):
    m = tas(ctx, 8602)
    bodies = [args(lab("test-policy"), NODES[:4]), args(lab("panics"), NODES[:4]),
              args(lab("less"), NODES[:4])]
    with pytest.raises(ext.HandlerPanic) as single:
        [m.filter(b) for b in bodies]
    with pytest.raises(ext.HandlerPanic) as batch:
        m.filter_batch(bodies)
    assert str(batch.value) == str(single.value)
    # Violated runs before the empty-list check: an empty node list panics too
    with pytest.raises(ext.HandlerPanic):
        m.filter_batch([bodies[0], args(lab("panics"), [])])
    # prioritize never evaluates dontschedule rules
    assert m.prioritize_batch(bodies) == [m.prioritize(b) for b in bodies]


KINDS = ["gpu.intel.com/i915", "gpu.intel.com/memory.max"]


def gas_cluster():
    names = [f"gpu-{i}" for i in range(9)]
    nodes = []
    for i in range(9):
        if i == 4:
            nodes.append({"labels": {}, "allocatable": {}})  # no cards label
            continue
        cards = ".".join(f"card{c}" for c in range(1 + i % 4))
        nodes.append({"labels": {"gpu.intel.com/cards": cards},
                      "allocatable": {"gpu.intel.com/i915": str(1 + i % 4),
                                      "gpu.intel.com/memory.max": f"{4 * (1 + i % 4)}G"}})
    return names, nodes


def gas_body(pod, names, key_case=str):
    a = {"Pod": pod, "NodeNames": list(names)}
    return json.dumps({key_case(k): v for k, v in a.items()}).encode()


def test_gas_filter_batch_is_byte_equal_to_the_single_verb(ctx):
    names, nodes = gas_cluster()
    n_cards, cap, used, card_names = sn.gas_snapshot_from_nodes(nodes, KINDS)
    ctx.gas_snapshot_set(8610, n_cards, cap, used)
    g = ext.GASExtender(ctx, 8610, names, card_names, KINDS)
    two = gas_pod("two", mem="2G")
    two["spec"]["containers"].append({"resources": {"requests": {
        "gpu.intel.com/i915": "2", "gpu.intel.com/memory.max": "6G"}}})
    odd = gas_pod("odd")
    odd["spec"]["containers"][0]["resources"]["requests"]["gpu.intel.com/tiles"] = "1"
    plain = {"metadata": {"name": "plain", "namespace": "default"},
             "spec": {"containers": [{"resources": {"requests": {"cpu": "1"}}}]}}
    bodies = [
        b"",                                                  # decode error
        b"{\"Pod\": {",                                       # decode error (truncated)
        gas_body(gas_pod("p0"), []),                          # no nodes
        gas_body(gas_pod("p0"), names),
        gas_body(gas_pod("p1", mem="3G", i915="1"), names[::-1]),
        gas_body(gas_pod("p2", mem="30G", i915="1"), names),  # fits nowhere
        gas_body(two, names[2:] + ["ghost", "gpu-0"]),        # a node the snapshot lacks
        gas_body(two, ["gpu-3", "gpu-3", "gpu-1", "gpu-3"]),  # a repeated name
        gas_body(odd, names),                                 # a kind no node has
        gas_body(plain, names, key_case=str.lower),           # no GPU request
        gas_body(gas_pod("p3", mem="8G", i915="4"), names),
        gas_body(gas_pod("p4"), ["ghost"]),
    ]
    want = [g.filter(b) for b in bodies]
    assert g.filter_batch(bodies) == want
    assert (404, b"") in want and {w[0] for w in want} == {200, 404}
    fits = [json.loads(w[1])["NodeNames"] for w in want if w[0] == 200]
    assert any(f is None for f in fits) and any(f and len(f) < 9 for f in fits)
    assert g.filter_batch([]) == [] and g.filter_batch(bodies[:3]) == want[:3]
