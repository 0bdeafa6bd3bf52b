"""TasCache.compact and GasCache.compact: the caches drop their dead node slots.

TasCache alone: two refreshes leave 80 slots that no metric lists; after compact(spare_nodes=64)
the extender's batch verbs answer the same, by name, for the live nodes.  GasCache with a
TasCache over its slots: deleted nodes go unless they still hold usage, both snapshots keep
equal node counts, and a batch placed to completion lands on the same nodes, by name, as on
caches built from scratch with the surviving nodes."""
import itertools

import numpy as np
import pytest

from pas_amd import _lib
from pas_amd import extender as ext
from pas_amd.context import RULE_DTYPE
from pas_amd.gas_cache import OK, GasCache
from pas_amd.tas_cache import TasCache
from test_extender import args
from test_gas_cache_nodes import KINDS, node_obj, pod_obj

pytestmark = pytest.mark.gpu

_gen = itertools.count(0x5CA0000, 0x1000)
POLICIES = {
    ("default", "up"): {"scheduleonmetric": [("load", "GreaterThan", 0)],
                        "dontschedule": [("load", "GreaterThan", 7), ("temp", "LessThan", 2)]},
    ("default", "down"): {"scheduleonmetric": [("temp", "LessThan", 0)],
                          "dontschedule": [("temp", "Equals", 5)]},
}


def maps(names, salt):
    """Two metric maps over `names` with few distinct values (ties), "temp" missing here and
    there."""
    load = {n: str((int(n[1:]) * 7 + salt) % 10) for n in names}
    temp = {n: str((int(n[1:]) * 3 + salt) % 8) for n in names if int(n[1:]) % 9 != 4}
    return {"load": load, "temp": temp}


def test_tas_cache_compact_keeps_the_answers(ctx):
    gen = next(_gen)
    first = [f"n{i:03d}" for i in range(200)]
    tas = TasCache.from_metrics(ctx, gen, maps(first, 0))
    for name in ("load", "temp"):
        tas.write_metric(name)  # registered: the refresh fetches it
    live = [n for i, n in enumerate(first) if i % 5 not in (1, 3)] + \
        [f"n{i:03d}" for i in range(300, 310)]
    assert len(live) == 130
    second = maps(live, 1)
    tas.update_all_metrics(second.__getitem__)
    assert len(tas.node_names) > 200 and set(first) <= set(tas.node_index)
    m = ext.MetricsExtender(ctx, tas.gen, first, ["load", "temp"], POLICIES)
    m.snapshot_changed(tas.gen, tas.node_names, tas.metric_names)
    bodies = [args({"telemetry-policy": "up"}, live),
              args({"telemetry-policy": "up"}, live[::-1]),
              args({"telemetry-policy": "down"}, live[5:90:3] + live[:4]),
              args({"telemetry-policy": "down"}, live[100:])]
    want = m.filter_batch(bodies), m.prioritize_batch(bodies)
    assert all(status == 200 and body for status, body in want[0] + want[1])

    src = tas.compact(spare_nodes=64)
    assert len(src) == len(tas.node_names) == 130 + 64
    assert ctx.tas_snapshot_info()[:2] == (tas.gen, 194)
    assert tas.node_names[130:] == [None] * 64 and set(tas.node_index) == set(live)
    # the live slots in their old order
    kept = [s for s in src if s >= 0]
    assert kept == sorted(kept) and len(kept) == 130
    m.snapshot_changed(tas.gen, tas.node_names, tas.metric_names)
    assert (m.filter_batch(bodies), m.prioritize_batch(bodies)) == want

    # a dropped name that comes back takes a fresh slot
    back = "n001"
    assert back not in tas.node_index
    third = maps(live + [back], 2)
    tas.update_all_metrics(third.__getitem__)
    assert tas.node_index[back] == 130 and len(tas.node_names) == 194
    m.snapshot_changed(tas.gen, tas.node_names, tas.metric_names)
    status, body = m.prioritize(args({"telemetry-policy": "up"}, live + [back]))
    assert status == 200 and back.encode() in body
    # and nothing is left to drop but the spare slots
    assert [s for s in tas.compact() if s >= 0] == list(range(131))


def place(ctx, tas, gas, n_pods=12, k=4):
    """A small batch placed to completion on the caches' snapshots: the nodes by name."""
    import torch
    from pas_amd.placement import place_to_completion
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    load, temp = tas.metric_index["load"], tas.metric_index["temp"]
    less, greater = _lib.PAS_OP_LESS_THAN, _lib.PAS_OP_GREATER_THAN
    rules = np.array([(temp, less, 1)] * n_pods, RULE_DTYPE)  # dontschedule: temp LessThan 1
    off = np.arange(n_pods + 1, dtype=np.int32)
    prio = np.array([(load, greater, 0) if p % 3 else (temp, less, 0) for p in range(n_pods)],
                    RULE_DTYPE)
    req = np.zeros((n_pods, 1, len(KINDS)), np.int64)
    req[:, 0] = (1, 1500)
    mask = np.full((n_pods, 1), 0b11, np.uint32)
    r = place_to_completion(ctx, tas.gen, gas.gen, n_pods, n_pods, dev(rules.view(np.uint8)),
                            dev(off), dev(prio.view(np.uint8)), None, 1, 0, dev(req),
                            dev(mask.view(np.int32)), dev(np.ones(n_pods, np.int32)), k)
    gas.gen = r.gas_gen
    return [gas.node_names[n] if n >= 0 else None for n in r.node.cpu().numpy()]


def test_gas_and_tas_caches_compact_together(ctx):
    gen = next(_gen)
    names = [f"g{i:03d}" for i in range(150)]
    nodes = {n: node_obj(n, ["card0", "card1"]) for n in names}
    metrics = maps(names, 3)
    gas = GasCache.from_nodes(ctx, gen, list(nodes.values()), KINDS)
    tas = TasCache.from_metrics(ctx, gen + 0x800, metrics, slots=gas)
    deleted = names[3:150:4][:35] + names[4:24:4]  # 35 idle ones, 5 that hold a pod
    assert len(set(deleted)) == 40
    busy = deleted[35:]
    pods = [pod_obj(f"pod-{n}", n, [(1, 1000)], annotation="card1") for n in busy + names[:2]]
    for pod in pods:
        gas.add_pod(pod)
    assert [o for _, _, o in gas.flush()] == [OK] * len(pods)
    for n in deleted:
        gas.delete_node(nodes[n])
    assert [o for _, _, o in gas.flush()] == [OK] * 40
    _, used0 = ctx.gas_snapshot_get()
    slot0 = dict(gas.node_index)

    with pytest.raises(ValueError):
        tas.compact()  # the slot owner decides
    src = gas.compact()
    assert tas.compact(src) == src
    # the 35 go, the 5 stay with their usage
    assert len(src) == len(gas.node_names) == 115 and -1 not in src
    assert set(gas.node_index) == set(names) - set(deleted[:35])
    assert gas.node_names == tas.node_names
    assert ctx.gas_snapshot_info()[:2] == (gas.gen, 115)
    assert ctx.tas_snapshot_info()[:2] == (tas.gen, 115)
    _, n_cards, _ = ctx.gas_snapshot_get_nodes()
    _, used = ctx.gas_snapshot_get()
    for n in busy:
        assert n_cards[gas.node_index[n]] == -1 and used[gas.node_index[n]].any()
    for n, at in gas.node_index.items():
        np.testing.assert_array_equal(used[at], used0[slot0[n]])
    np.testing.assert_array_equal(gas.n_cards, n_cards)
    assert [len(c) for c in gas.card_names] == [max(int(c), 0) for c in n_cards]
    assert tas.skipped_nodes == set(deleted[:35])
    got = place(ctx, tas, gas)
    assert len(set(got)) > 1 and None not in got and not set(got) & set(deleted)

    # the same on caches built from scratch with the surviving nodes
    alive = [n for n in names if n not in deleted]
    gas2 = GasCache.from_nodes(ctx, gen + 0x100, [nodes[n] for n in alive], KINDS)
    for pod in pods[len(busy):]:
        gas2.add_pod(pod)
    assert [o for _, _, o in gas2.flush()] == [OK] * 2
    tas2 = TasCache.from_metrics(ctx, gen + 0x900, metrics, slots=gas2)
    assert place(ctx, tas2, gas2) == got
