"""GasCache node events (pas_amd/gas_cache.py add_node / update_node / delete_node) and
snapshot.card_remap.

The checker of the GPU part is a dict model of the reference: a lister {name: node} and
nodeStatuses[name][card] = {kind: usage} (node_resource_cache.go:64,259-272), which never forgets
a node or a card.  Arrays are built from the model from scratch, in slot order, with
gas_snapshot_from_nodes, and the oracle's fit / bind run on those arrays.  The generated
sequences stay inside the documented divergences, and assert so on themselves: a pod event
names only cards the label lists at that point, and label + parked cards never pass max_cards.

The CPU part needs no GPU: card_remap, the order in which flush() plans its calls (against a
recording context), and the header."""
import json

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib, extender, snapshot
from pas_amd.gas_cache import (NODE_ADDED, NODE_DELETED, NODE_UPDATED, OK, POD_ADDED,
                               POD_COMPLETED, GasCache)
from pas_amd.snapshot import GPU_LIST_LABEL, card_remap

KINDS = ["gpu.intel.com/i915", "gpu.intel.com/memory.max"]
Q = len(KINDS)


def node_obj(name, cards, i915_per=4, mem_per=4000):
    """A v1.Node: `cards` label cards (None: no label), allocatable = per-card share x cards."""
    labels = {} if cards is None else {GPU_LIST_LABEL: ".".join(cards)}
    n = max(len(cards or []), 1)
    return {"metadata": {"name": name, "labels": labels},
            "status": {"allocatable": {KINDS[0]: str(i915_per * n), KINDS[1]: str(mem_per * n)}}}


def pod_obj(name, node, containers, annotation=None, phase="Running"):
    """containers: [(numI915, memory)]."""
    meta = {"namespace": "default", "name": name}
    if annotation is not None:
        meta["annotations"] = {"gas-container-cards": annotation}
    spec = {"nodeName": node, "containers": [
        {"name": f"c{i}", "resources": {"requests": {KINDS[0]: str(a), KINDS[1]: str(b)}}}
        for i, (a, b) in enumerate(containers)]}
    return {"metadata": meta, "spec": spec, "status": {"phase": phase}}


# ------------------------------------------------------------------ CPU: card_remap

def test_card_remap_leave_and_return():
    old = ["card0", "card1", "card2"]
    src, slots, dropped = card_remap(old, ["card0", "card2"], 4)
    assert (src, slots, dropped) == ([0, 2, 1, -1], ["card0", "card2", "card1"], [])
    # card1 returns to its rank with its slot; a card first seen starts at zero
    src, slots, dropped = card_remap(slots, ["card0", "card1", "card2", "card3"], 4)
    assert (src, slots, dropped) == ([0, 2, 1, -1], ["card0", "card1", "card2", "card3"], [])
    # no label (or a deleted node): everything is parked where it is
    assert card_remap(old, [], 4) == ([0, 1, 2, -1], old, [])
    assert card_remap([], [], 2) == ([-1, -1], [], [])


def test_card_remap_orders_like_sort_strings():
    # sort.Strings is bytewise: "card10" < "card2"; duplicates in the label count once
    src, slots, dropped = card_remap(["card2", "card9"], ["card9", "card10", "card2", "card2"], 8)
    assert slots == ["card10", "card2", "card9"] and dropped == []
    assert src == [-1, 0, 1] + [-1] * 5


def test_card_remap_overflow_keeps_the_most_recently_parked():
    old = ["a", "b", "c", "d", "p1", "p2"]  # p1 was parked after p2
    src, slots, dropped = card_remap(old, ["a", "x", "y", "z"], 6)
    # b, c, d just left: they stand before p1, p2; two parked slots are left
    assert slots == ["a", "x", "y", "z", "b", "c"] and dropped == ["d", "p1", "p2"]
    assert src == [0, -1, -1, -1, 1, 2]
    with pytest.raises(ValueError):
        card_remap(old, list("abcdefg"), 6)  # the label alone does not fit: grow first


# ------------------------------------------------------------------ CPU: flush() planning

class RecordingCtx:
    """Records the device calls GasCache plans, in order; every status is OK."""

    def __init__(self, shape):
        self.gas_shape = shape
        self.calls = []

    def gas_apply(self, gen_from, gen_to, kinds, pods, nodes, req, mask, ncont, cpc, cards):
        self.calls.append(("apply", gen_from, gen_to, list(kinds), list(nodes),
                           np.array(cards).tolist()))
        return np.zeros(len(kinds), np.int32)

    def gas_nodes_update(self, gen_from, gen_to, nodes, n_cards, cap, src):
        self.calls.append(("nodes", gen_from, gen_to, list(nodes), list(n_cards),
                           np.array(cap).tolist(), np.array(src).tolist()))
        return np.zeros(len(nodes), np.int32)

    def gas_snapshot_resize(self, gen_from, gen_to, n_nodes, max_cards):
        self.calls.append(("resize", gen_from, gen_to, n_nodes, max_cards))
        self.gas_shape = (n_nodes, max_cards, self.gas_shape[2])

    def gas_snapshot_set(self, gen, n_cards, cap, used):
        self.calls.append(("set", gen, np.array(n_cards).tolist(), np.array(used).shape))


def planning_cache():
    names = ["node-a", "node-b", None]  # one spare slot
    cards = [["card0", "card1", "card2"], ["card0"], []]
    ctx = RecordingCtx((3, 4, Q))
    gc = GasCache(ctx, 100, names, cards, KINDS, n_cards=np.array([3, 1, -1], np.int32),
                  cap=np.array([[4, 4000], [4, 4000], [0, 0]], np.int64))
    return ctx, gc, cards


def test_flush_keeps_the_informer_order():
    ctx, gc, cards = planning_cache()
    gc.add_pod(pod_obj("p1", "node-a", [(1, 100)], "card2"))
    gc.update_node(None, node_obj("node-a", ["card1", "card2"]))   # card0 leaves
    gc.add_node(node_obj("node-c", ["card0", "card1"]))            # takes the spare slot
    gc.update_node(None, node_obj("node-a", ["card0", "card2"]))   # node-a again, same batch
    gc.add_pod(pod_obj("p2", "node-a", [(1, 100)], "card2"))       # ranks as of this point
    gc.add_pod(pod_obj("p3", "node-c", [(1, 100)], "card1"))
    gc.delete_node(node_obj("node-b", None))
    gc.delete_node(node_obj("nobody", None))                        # never held: no call
    assert ctx.calls == []  # handlers only queue
    assert gc.flush() == [
        ("default&p1", POD_ADDED, OK), ("node-a", NODE_UPDATED, OK), ("node-c", NODE_ADDED, OK),
        ("node-a", NODE_UPDATED, OK), ("default&p2", POD_ADDED, OK),
        ("default&p3", POD_ADDED, OK), ("node-b", NODE_DELETED, OK),
        ("nobody", NODE_DELETED, OK)]
    assert ctx.calls == [
        ("apply", 100, 101, [0], [0], [[2]]),               # card2 was rank 2
        ("nodes", 101, 102, [0, 2, 0], [2, 2, 2],
         [[4, 4000], [4, 4000], [4, 4000]],
         # card1, card2 | card0 parked; the spare slot's new cards; card0, card2 | card1 parked
         [[1, 2, 0, -1], [-1, -1, -1, -1], [2, 1, 0, -1]]),
        ("apply", 102, 103, [0, 0], [0, 2], [[1], [1]]),    # card2 is rank 1 now
        ("nodes", 103, 104, [1], [-1], [[0, 0]], [[0, 1, 2, 3]]),
    ]
    assert gc.gen == 104
    assert gc.node_names == ["node-a", "node-b", "node-c"]
    assert cards == [["card0", "card2"], [], ["card0", "card1"]]    # changed in place
    assert gc.card_names is cards
    assert gc.parked == [["card1"], ["card0"], []]
    np.testing.assert_array_equal(gc.n_cards, [2, -1, 2])
    np.testing.assert_array_equal(gc.cap, [[4, 4000], [0, 0], [4, 4000]])


def test_flush_grows_before_the_update_that_needs_it():
    ctx, gc, cards = planning_cache()
    gc.add_node(node_obj("node-c", ["card0"]))                      # the spare slot
    gc.add_node(node_obj("node-d", ["card0"]))                      # none left: 3 -> 67 slots
    gc.update_node(None, node_obj("node-d", [f"card{i}" for i in range(5)]))  # 5 > 4: 8 cards
    results = gc.flush()
    assert [r[2] for r in results] == [OK, OK, OK]
    assert [c[0] for c in ctx.calls] == ["nodes", "resize", "nodes", "resize", "nodes"]
    assert ctx.calls[1] == ("resize", 101, 102, 67, 4)
    assert ctx.calls[2][3:5] == ([3], [1])
    assert ctx.calls[3] == ("resize", 103, 104, 67, 8)
    assert ctx.calls[4][3:5] == ([3], [5]) and ctx.calls[4][6] == [[0, -1, -1, -1, -1, -1, -1, -1]]
    assert gc.gen == 105 and gc.max_cards == 8 and len(gc.node_names) == 67 == len(cards)
    assert gc.n_cards.shape == (67,) and gc.cap.shape == (67, Q)
    # rebuild keeps the current slots and pitch
    gc.rebuild([])
    assert ctx.calls[-1] == ("set", 106, gc.n_cards.tolist(), (67, 8, Q))


def test_parking_overflow_is_reported():
    ctx = RecordingCtx((1, 4, Q))
    gc = GasCache(ctx, 7, ["n"], [["c0", "c1", "c2"]], KINDS)
    gc.update_node(None, node_obj("n", ["c0", "x", "y"]))
    assert gc.flush() == [("n", NODE_UPDATED, "dropped: c2")]
    assert ctx.calls[0][6] == [[0, -1, -1, 1]] and gc.parked == [["c1"]]


def test_header_declares_the_node_entry_points():
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in ("pas_gas_nodes_update", "pas_gas_nodes_update_device", "pas_gas_snapshot_resize",
                 "pas_gas_snapshot_info", "pas_gas_snapshot_get_nodes"):
        assert f"int {name}(" in header
        assert name in _lib.SIGNATURES
        assert getattr(pas_amd.LIB, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["pas_gas_nodes_update_device"][1]) == \
        len(_lib.SIGNATURES["pas_gas_nodes_update"][1]) + 1  # + hip_stream
    assert "#define PAS_ABI_VERSION 3" in header and "#define PAS_K_COUNT 10" in header
    for method in ("gas_nodes_update", "gas_nodes_update_device", "gas_snapshot_resize",
                   "gas_snapshot_info", "gas_snapshot_get_nodes"):
        assert callable(getattr(pas_amd.Context, method))


# ------------------------------------------------------------------ the dict model

class Model:
    """The reference's view: the lister and nodeStatuses, keyed by names, never deleted."""

    def __init__(self):
        self.lister = {}
        self.statuses = {}

    def label(self, name):
        node = self.lister.get(name)
        text = ((node or {}).get("metadata") or {}).get("labels", {}).get(GPU_LIST_LABEL)
        return [] if text is None else snapshot.go_sort_strings(set(text.split(".")))

    def adjust(self, pod, annotation, sign):
        """adjustPodResources (node_resource_cache.go:240-287) on cards the label lists."""
        usage = self.statuses.setdefault(pod["spec"]["nodeName"], {})
        for cont, segment in zip(pod["spec"]["containers"], annotation.split("|")):
            names = segment.split(",") if segment else []
            for card in names:
                per_card = usage.setdefault(card, {k: 0 for k in KINDS})
                for kind, text in cont["resources"]["requests"].items():
                    per_card[kind] = max(per_card[kind] + sign * (int(text) // len(names)), 0)

    def arrays(self, slot_names):
        """(n_cards, cap, used, card_names) from scratch, in slot order."""
        nodes = []
        for name in slot_names:
            node = self.lister.get(name) if name is not None else None
            nodes.append(None if node is None else
                         {"labels": node["metadata"]["labels"],
                          "allocatable": node["status"]["allocatable"],
                          "usage": self.statuses.get(name, {})})
        return snapshot.gas_snapshot_from_nodes(nodes, KINDS)


def probe_pods(seed, n=16, c=2):
    rng = np.random.default_rng(seed)
    req = np.zeros((n, c, Q), np.int64)
    req[:, :, 0] = rng.choice([0, 1, 2], size=(n, c), p=[0.1, 0.7, 0.2])
    req[:, :, 1] = rng.integers(100, 5000, size=(n, c))
    ncont = rng.integers(1, c + 1, size=n).astype(np.int32)
    mask = np.where(req[:, :, 0] > 0, 3, 2).astype(np.uint32)
    live = np.arange(c)[None, :] < ncont[:, None]
    mask[~live] = 0
    req[~live] = 0
    return req, mask, ncont


def check_fits(ctx, oracle, gc, model, probes):
    n_cards, cap, used, names = model.arrays(gc.node_names)
    got = ctx.gas_fit(gc.gen, *probes, 0)
    want = oracle.gas_fit(n_cards, cap, used, *probes, 0)
    np.testing.assert_array_equal(got, want)
    assert [list(c) for c in gc.card_names] == names
    return n_cards, cap, used, names


# ------------------------------------------------------------------ GPU: the interleaving

UNIVERSE = [f"card{i}" for i in (0, 1, 10, 2, 3, 4, 5, 6)]  # 8 names: parking always fits K = 8


def drive(ctx, oracle, seed, n_items=400):
    rng = np.random.default_rng(seed)
    model = Model()
    k = 8

    def fresh_node(name):
        return node_obj(name, list(rng.choice(UNIVERSE, size=rng.integers(1, 7), replace=False)),
                        i915_per=int(rng.integers(2, 6)), mem_per=int(rng.integers(2000, 9000)))

    start = [fresh_node(f"node-{i:02d}") for i in range(56)]
    for node in start:
        model.lister[node["metadata"]["name"]] = node
    gc = GasCache.from_nodes(ctx, 70000 + 1000 * seed, start, KINDS, spare_nodes=6)
    ever = {name: set(model.label(name)) for name in model.lister}  # every card ever listed
    pods, ext_pods = {}, {}
    ext = extender.GASExtender(ctx, gc.gen, [n or "" for n in gc.node_names],
                                       gc.card_names, KINDS, ext_pods)
    probes = probe_pods(seed)
    n_new, n_pod, n_node, touched, binds = 0, 0, 0, [], 0
    check_fits(ctx, oracle, gc, model, probes)
    for item in range(n_items):
        if rng.random() < 0.15:  # ---- a node item
            n_node += 1
            listed = sorted(model.lister)
            gone = sorted(set(ever) - set(model.lister))
            what = str(rng.choice(["add", "delete", "readd", "label", "alloc", "nolabel"]))
            if what == "delete" and len(listed) > 40:
                gc.delete_node(model.lister.pop(str(rng.choice(listed))))
            elif (what == "add" and n_new < 5) or (what == "readd" and gone):
                if what == "add":
                    node = fresh_node(f"late-{n_new}")
                    n_new += 1
                else:
                    node = fresh_node(str(rng.choice(gone)))
                name = node["metadata"]["name"]
                model.lister[name] = node
                ever.setdefault(name, set()).update(model.label(name))
                gc.add_node(node)
                touched.append(name)
            else:
                name = str(rng.choice(listed))
                old = model.lister[name]
                if what == "alloc":
                    node = node_obj(name, model.label(name) or None, int(rng.integers(2, 6)),
                                    int(rng.integers(2000, 9000)))
                elif what == "nolabel":
                    node = node_obj(name, None)
                else:  # the label shrinks or grows
                    node = fresh_node(name)
                model.lister[name] = node
                gc.update_node(old, node)
                ever[name] |= set(model.label(name))
                touched.append(name)
        else:  # ---- a pod item
            n_pod += 1
            done = [key for key, (pod, ann) in pods.items()
                    if all(card in model.label(pod["spec"]["nodeName"])
                           for seg in ann.split("|") for card in seg.split(",") if card)]
            if done and rng.random() < 0.4:
                pod, ann = pods.pop(done[int(rng.integers(len(done)))])
                gone_pod = json.loads(json.dumps(pod))
                gone_pod["status"]["phase"] = "Succeeded"
                model.adjust(pod, ann, -1)
                gc.update_pod(pod, gone_pod)
            else:
                labelled = [n for n in sorted(model.lister) if model.label(n)]
                name = str(rng.choice(labelled))
                label = model.label(name)
                conts = [(int(rng.integers(1, 3)), int(rng.integers(100, 3000)))
                         for _ in range(rng.integers(1, 3))]
                # every card a pod event names is in the label at this point of the queue
                ann = "|".join(",".join(rng.choice(label, size=min(a, len(label)), replace=False))
                               for a, _ in conts)
                assert all(card in label for seg in ann.split("|") for card in seg.split(","))
                pod = pod_obj(f"pod-{item}", name, conts, ann)
                pods[f"pod-{item}"] = (pod, ann)
                model.adjust(pod, ann, +1)
                gc.add_pod(pod)
        # label + parked cards never pass max_cards (no card is dropped)
        assert all(len(cards) <= k for cards in ever.values())
        if item % 25 == 24 or item == n_items - 1:
            results = gc.flush()
            assert [r for r in results if r[2] != OK] == []
            assert {r[1] for r in results} <= {POD_ADDED, POD_COMPLETED, NODE_ADDED,
                                               NODE_UPDATED, NODE_DELETED}
            n_cards, cap, used, names = check_fits(ctx, oracle, gc, model, probes)
            # a bind through the extender on a node the events touched
            target = next((n for n in reversed(touched) if model.label(n)), None)
            if target is not None:
                ext.nodes_changed(gc.node_names)
                ext.gen = gc.gen
                pod = pod_obj(f"bound-{item}", target, [(1, 500), (2, 300)])
                ext_pods[("default", pod["metadata"]["name"])] = pod
                status, _ = ext.bind(json.dumps({"PodName": pod["metadata"]["name"],
                                                 "PodNamespace": "default",
                                                 "Node": target}).encode())
                gc.gen = ext.gen
                slot = gc.node_index[target]
                breq = np.array([[[1, 500], [2, 300]]], np.int64)
                _, _, w_st, w_cnt = oracle.gas_bind(n_cards, cap, used, breq,
                                                    np.array([[3, 3]], np.uint32),
                                                    np.array([2], np.int32), 0, [0], [slot],
                                                    counts=True)
                assert (status == 200) == (w_st[0] == _lib.PAS_GAS_OK)
                if status == 200:
                    binds += 1
                    ann = pod["metadata"]["annotations"]["gas-container-cards"]
                    assert ann == snapshot.annotation_counts(w_cnt[0], 2, model.label(target))
                    model.adjust(pod, ann, +1)
                    gc.note_bind(pod, ann)
                    check_fits(ctx, oracle, gc, model, probes)
            touched.clear()
    return gc, model, n_pod, n_node, binds


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_interleaved_pod_and_node_events_match_the_model(ctx, oracle, seed):
    gc, model, n_pod, n_node, binds = drive(ctx, oracle, seed)
    assert n_node >= 40 and n_pod >= 300 and binds >= 1
    assert gc.max_cards == 8 and len(gc.node_names) == 62  # 5 late nodes fit the 6 spare slots
    # the usage never left the device: what it holds is the model's, label cards and parked
    _, used = ctx.gas_snapshot_get()
    for slot, name in enumerate(gc.node_names):
        slots = list(gc.card_names[slot]) + gc.parked[slot]
        for r in range(8):
            want = model.statuses.get(name, {}).get(slots[r], {}) if r < len(slots) else {}
            assert list(used[slot, r]) == [want.get(kind, 0) for kind in KINDS], (name, r)


@pytest.mark.gpu
def test_parking_overflow_drops_the_oldest_parked_cards(ctx, oracle):
    model = Model()
    node = node_obj("n0", [f"c{i}" for i in range(6)])
    model.lister["n0"] = node
    gc = GasCache.from_nodes(ctx, 76000, [node], KINDS)
    assert gc.max_cards == 8
    for i in (1, 4):
        pod = pod_obj(f"p{i}", "n0", [(1, 100 * i)], f"c{i}")
        model.adjust(pod, f"c{i}", +1)
        gc.add_pod(pod)
    # five cards leave a six-card label of an eight-slot row: two are parked, three dropped
    gc.update_node(node, node_obj("n0", ["c0", "d0", "d1", "d2", "d3", "d4"]))
    assert gc.flush()[-1] == ("n0", NODE_UPDATED, "dropped: c3, c4, c5")
    assert gc.parked == [["c1", "c2"]]
    # c1 returns with its usage; c4 returns empty, where the reference would remember it
    back = node_obj("n0", ["c0", "c1", "c4"])
    gc.update_node(None, back)
    assert gc.flush() == [("n0", NODE_UPDATED, "dropped: c2")]  # (c2 never had usage)
    model.lister["n0"] = back
    del model.statuses["n0"]["c4"]  # the documented divergence
    check_fits(ctx, oracle, gc, model, probe_pods(3))
    _, used = ctx.gas_snapshot_get()
    np.testing.assert_array_equal(used[0, :3], [[0, 0], [1, 100], [0, 0]])
    assert not used[0, 3:].any()


@pytest.mark.gpu
def test_both_kinds_of_growth(ctx, oracle):
    model = Model()
    start = [node_obj(f"s{i}", ["card0", "card1", "card2"]) for i in range(3)]
    for node in start:
        model.lister[node["metadata"]["name"]] = node
    gc = GasCache.from_nodes(ctx, 78000, start, KINDS, spare_nodes=2)
    ext = extender.GASExtender(ctx, gc.gen, [n or "" for n in gc.node_names],
                                       gc.card_names, KINDS, {})
    probes = probe_pods(9)
    assert ctx.gas_shape == (5, 8, Q)
    pod = pod_obj("p", "s1", [(2, 1000)], "card2,card0")
    model.adjust(pod, "card2,card0", +1)
    gc.add_pod(pod)
    for i in range(5):  # two spare slots, then the snapshot grows by 64 slots
        node = node_obj(f"late{i}", ["card0", "card1"])
        model.lister[f"late{i}"] = node
        gc.add_node(node)
    wide = node_obj("late1", [f"card{i}" for i in range(9)])  # 9 cards at K = 8: 16
    model.lister["late1"] = wide
    gc.update_node(None, wide)
    pod = pod_obj("q", "late1", [(1, 700)], "card8")
    model.adjust(pod, "card8", +1)
    gc.add_pod(pod)
    assert [r[2] for r in gc.flush()] == [OK] * 8
    assert ctx.gas_shape == (69, 16, Q) and ctx.gas_snapshot_info()[1:] == (69, 16, Q)
    assert gc.node_names[:8] == ["s0", "s1", "s2"] + [f"late{i}" for i in range(5)]
    assert gc.node_names[8:] == [None] * 61 and ext.card_names is gc.card_names
    check_fits(ctx, oracle, gc, model, probes)
    ext.nodes_changed(gc.node_names)
    assert ext.node_index["late4"] == 7 and len(ext.card_names) == 69
    # rebuild keeps working on the current slots: the same usage from the pods' annotations
    results = gc.rebuild([pod_obj("p", "s1", [(2, 1000)], "card2,card0"),
                          pod_obj("q", "late1", [(1, 700)], "card8")])
    assert [r[2] for r in results] == [OK, OK] and ctx.gas_shape == (69, 16, Q)
    check_fits(ctx, oracle, gc, model, probes)
