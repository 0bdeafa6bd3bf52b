"""MetricsExtender over a PolicyCache (the resident policy table) against MetricsExtender over
the equivalent dict: filter, prioritize, filter_batch and prioritize_batch answer identical
(status, body) for test_extender_batch.py's request mix, the 404 and 400 paths and the
handler's panic included."""
import pytest

from pas_amd import extender as ext
from pas_amd import snapshot as sn
from pas_amd.policy_cache import PolicyCache, TasPolicy
from test_extender import args
from test_extender_batch import NODES, POLICIES, lab, tas_bodies

pytestmark = pytest.mark.gpu

METRICS = ["dummyMetric1", "second", "emptyMetric"]


def extenders(ctx, gen):
    """(over the dict, over a PolicyCache fed by onAdd events) on one snapshot."""
    m1 = {n: str(10 * (i % 3)) for i, n in enumerate(NODES) if i % 11 != 5}
    m2 = {n: str(i % 8) for i, n in enumerate(NODES) if i % 7 != 3}
    v, pres, scale = sn.tas_snapshot_from_metrics(
        {"dummyMetric1": m1, "second": m2, "emptyMetric": {}}, NODES, METRICS)
    ctx.tas_snapshot_set(gen, v, pres, scale)
    cache = PolicyCache(ctx, metric_names=METRICS)
    for (ns, name), strategies in POLICIES.items():
        cache.on_add(TasPolicy(ns, name, strategies))
    assert ctx.tas_policies_info()[0] == len(POLICIES)
    return (ext.MetricsExtender(ctx, gen, NODES, METRICS, POLICIES),
            ext.MetricsExtender(ctx, gen, NODES, METRICS, cache))


def test_every_verb_answers_as_over_the_dict(ctx):
    by_dict, by_cache = extenders(ctx, 8700)
    bodies = tas_bodies() + [args({"useless-label": "x"}, [])]
    want_f = [by_dict.filter(b) for b in bodies]
    want_p = [by_dict.prioritize(b) for b in bodies]
    assert [by_cache.filter(b) for b in bodies] == want_f
    assert [by_cache.prioritize(b) for b in bodies] == want_p
    assert by_cache.filter_batch(bodies) == want_f == by_dict.filter_batch(bodies)
    assert by_cache.prioritize_batch(bodies) == want_p == by_dict.prioritize_batch(bodies)
    # every kind of answer is in the mix
    assert {w[0] for w in want_f} == {200, 404} and (404, b"null\n") in want_f
    assert {w[0] for w in want_p} == {200, 400} and (400, b"[]\n") in want_p
    assert any(w[0] == 200 and len(w[1]) > 10 for w in want_f)
    assert any(w[0] == 200 and len(w[1]) > 10 for w in want_p)
    assert by_cache.filter_batch([]) == [] and by_cache.prioritize_batch([]) == []
    assert by_cache.filter_batch(bodies[:4]) == want_f[:4]  # nothing left for the library


def test_the_panic_is_the_single_verbs(ctx):
    by_dict, by_cache = extenders(ctx, 8701)
    bodies = [args(lab("test-policy"), NODES[:4]), args(lab("panics"), NODES[:4]),
              args(lab("less"), NODES[:4])]
    with pytest.raises(ext.HandlerPanic) as single:
        [by_dict.filter(b) for b in bodies]
    with pytest.raises(ext.HandlerPanic) as batch:
        by_cache.filter_batch(bodies)
    assert str(batch.value) == str(single.value)
    # Violated runs before the empty-list check: an empty node list panics too
    with pytest.raises(ext.HandlerPanic):
        by_cache.filter_batch([bodies[0], args(lab("panics"), [])])
    # a batch that does not name the policy is answered
    ok = [bodies[0], bodies[2]]
    assert by_cache.filter_batch(ok) == [by_dict.filter(b) for b in ok]
    assert by_cache.prioritize_batch(bodies) == [by_dict.prioritize(b) for b in bodies]


def test_snapshot_changed_sets_the_table_again(ctx):
    # the columns in another order: the extender's hook re-resolves the cache's table too
    by_dict, by_cache = extenders(ctx, 8702)
    bodies = tas_bodies()
    moved = [METRICS[1], METRICS[0], METRICS[2]]
    ctx.tas_snapshot_reshape(8702, 8703, len(NODES), 3, [1, 0, 2])
    by_dict.snapshot_changed(8703, NODES, moved)
    by_cache.snapshot_changed(8703, NODES, moved)
    want = [by_dict.filter(b) for b in bodies]
    assert by_cache.filter_batch(bodies) == want
    assert by_cache.prioritize_batch(bodies) == [by_dict.prioritize(b) for b in bodies]
    assert any(w[0] == 200 and len(w[1]) > 10 for w in want)
