"""GasCache(device_events=True) against a stub context (no GPU): which device calls the cache
plans and in which order (the two tables installed, one names-form apply per pod batch, a row
update beside each node update, resize / remap beside the snapshot's), and that the host keeps
the annotatedPods bookkeeping of the default mode: skipped items, the podDeleted quirk, a batch
cut at a repeated key, the note_bind echo.  The stub answers the statuses the device would give
from snapshot.parse_annotation, so both modes can be driven side by side."""
import numpy as np
import pytest

from pas_amd import _lib, snapshot
from pas_amd.gas_cache import (BAD_ARGS, ERR_INPUT, NODE_ADDED, NODE_UPDATED, OK, POD_ADDED,
                               POD_COMPLETED, POD_DELETED, POD_UPDATED, SKIPPED, GasCache)
from test_gas_cache import pod
from test_gas_cache_nodes import KINDS, Q, node_obj, pod_obj

ADD, REMOVE = _lib.PAS_GAS_EV_ADD, _lib.PAS_GAS_EV_REMOVE


def unpack(off, blob):
    off = np.asarray(off)
    return [bytes(blob[off[i]:off[i + 1]]).decode() for i in range(len(off) - 1)]


class StubCtx:
    """Records the calls in order.  It keeps the two tables as Python lists, so that the
    names-form apply can answer what the device would: errBadArgs, the unknown node and the
    annotation without cards by the rules of pas.h, PAS_GAS_OK for every event that reaches the
    walker (or the scripted status)."""

    def __init__(self, shape, script=None):
        self.gas_shape = shape
        self.calls = []
        self.node_names, self.rows, self.k = None, None, None
        self.script = dict(script or {})  # pod index of a call -> status

    # -- the tables
    def names_set(self, off, blob):
        self.node_names = unpack(off, blob)
        self.calls.append(("names_set", list(self.node_names)))

    def names_assign(self, off, blob, new_cap=None, want_slots=True):
        names = unpack(off, blob)
        new_entry, new_slot = [], []
        for i, name in enumerate(names):
            if name and name not in self.node_names:
                slot = self.node_names.index("")  # the lowest spare slot
                self.node_names[slot] = name
                new_entry.append(i)
                new_slot.append(slot)
        self.calls.append(("names_assign", names, new_slot))
        return None, np.array(new_entry, np.int32), np.array(new_slot, np.int32)

    def names_resize(self, n_slots):
        self.node_names += [""] * (n_slots - len(self.node_names))
        self.calls.append(("names_resize", n_slots))

    def names_remap(self, src):
        self.node_names = [self.node_names[s] if s >= 0 else "" for s in src]
        self.calls.append(("names_remap", list(src)))

    def gas_card_names_set(self, n_slots, k, off, blob):
        flat = unpack(off, blob)
        assert len(flat) == n_slots * k
        self.k, self.rows = k, [flat[s * k:(s + 1) * k] for s in range(n_slots)]
        self.calls.append(("cards_set", n_slots, k, [list(r) for r in self.rows]))

    def gas_card_names_update(self, row_slot, off, blob):
        flat = unpack(off, blob)
        assert len(flat) == len(row_slot) * self.k
        for r, slot in enumerate(row_slot):
            self.rows[slot] = flat[r * self.k:(r + 1) * self.k]
        self.calls.append(("cards_update", list(row_slot),
                           [flat[r * self.k:(r + 1) * self.k] for r in range(len(row_slot))]))

    def gas_card_names_resize(self, n_slots, k):
        self.rows = [r + [""] * (k - self.k) for r in self.rows]
        self.rows += [[""] * k for _ in range(n_slots - len(self.rows))]
        self.k = k
        self.calls.append(("cards_resize", n_slots, k))

    def gas_card_names_remap(self, src):
        self.rows = [self.rows[s] if s >= 0 else [""] * self.k for s in src]
        self.calls.append(("cards_remap", list(src)))

    # -- the snapshot
    def gas_snapshot_set(self, gen, n_cards, cap, used):
        self.n_cards = np.array(n_cards)
        self.calls.append(("set", gen, np.array(used).shape))

    def gas_nodes_update(self, gen_from, gen_to, nodes, n_cards, cap, src):
        for n, c in zip(nodes, n_cards):
            self.n_cards[n] = c
        self.calls.append(("nodes", gen_from, gen_to, list(nodes), list(n_cards)))
        return np.zeros(len(nodes), np.int32)

    def gas_snapshot_resize(self, gen_from, gen_to, n_nodes, max_cards):
        self.n_cards = np.concatenate([self.n_cards, np.full(n_nodes - len(self.n_cards), -1)])
        self.gas_shape = (n_nodes, max_cards, self.gas_shape[2])
        self.calls.append(("resize", gen_from, gen_to, n_nodes, max_cards))

    def gas_snapshot_compact(self, gen_from, gen_to, src):
        self.n_cards = np.array([self.n_cards[s] if s >= 0 else -1 for s in src])
        self.gas_shape = (len(src),) + tuple(self.gas_shape[1:])
        self.calls.append(("compact", gen_from, gen_to, list(src)))

    def gas_snapshot_get_nodes(self):
        n, _, q = self.gas_shape
        return 0, self.n_cards.astype(np.int32), np.zeros((n, q), np.int64)

    def gas_snapshot_get(self):
        return 0, np.zeros(self.gas_shape, np.int64)

    # -- pod events
    def gas_apply(self, *a):
        raise AssertionError("device_events sends no pre-parsed batch")

    def gas_apply_annotations_names(self, gen_from, gen_to, kinds, pods, name_off, name_blob, req,
                                    mask, ncont, ann_off, ann_blob):
        nodes, anns = unpack(name_off, name_blob), unpack(ann_off, ann_blob)
        assert list(pods) == list(range(len(kinds)))
        st = []
        for e, (node, ann) in enumerate(zip(nodes, anns)):
            if len(ann.split("|")) != ncont[e] or node == "":
                st.append(_lib.PAS_GAS_ERR_BAD_ARGS)
            elif node not in self.node_names:
                st.append(_lib.PAS_GAS_OK)
            else:
                slot = self.node_names.index(node)
                label = self.rows[slot][:max(int(self.n_cards[slot]), 0)]
                _, ranks = snapshot.parse_annotation(ann, label)
                st.append(self.script.get((len(self.calls), e), _lib.PAS_GAS_OK) if ranks
                          else _lib.PAS_GAS_OK)
        self.calls.append(("apply_names", gen_from, gen_to, list(kinds), nodes, anns,
                           list(ncont)))
        return np.array(st, np.int32)


NAMES = ["node-a", "node-b", None]
CARDS = [["card0", "card1", "card2"], ["card0"], []]
N_CARDS = np.array([3, 1, -1], np.int32)
CAP = np.array([[4, 4000], [4, 4000], [0, 0]], np.int64)


def device_cache(script=None):
    ctx = StubCtx((3, 4, Q), script)
    ctx.n_cards = N_CARDS.copy()
    cards = [list(c) for c in CARDS]
    gc = GasCache(ctx, 100, NAMES, cards, KINDS, n_cards=N_CARDS, cap=CAP, device_events=True)
    return ctx, gc


def test_construction_installs_both_tables():
    ctx, gc = device_cache()
    assert ctx.calls == [
        ("cards_set", 3, 4, [["card0", "card1", "card2", ""], ["card0", "", "", ""],
                             ["", "", "", ""]]),
        ("names_set", ["node-a", "node-b", ""]),  # a spare slot is the empty name
    ]
    with pytest.raises(ValueError):
        GasCache(StubCtx((1, 4, Q)), 1, [""], [[]], KINDS, device_events=True)
    with pytest.raises(ValueError):
        gc.add_node(node_obj("", ["card0"]))
    # the default mode installs nothing and sends no string
    plain = StubCtx((3, 4, Q))
    GasCache(plain, 100, NAMES, [list(c) for c in CARDS], KINDS)
    assert plain.calls == []


def test_pack_card_names():
    off, blob = snapshot.pack_card_names([["b", "card10"], [], ["é"]], [["p"], [], []], 3)
    assert unpack(off, blob) == ["b", "card10", "p", "", "", "", "é", "", ""]
    assert off[-1] == len(blob) == len("bcard10pé".encode())
    with pytest.raises(ValueError):
        snapshot.pack_card_names([["a", "b"]], [["c"]], 2)
    assert snapshot.pack_card_names([], None, 4)[0].tolist() == [0]


def test_one_names_form_apply_per_batch_and_nothing_parsed_on_the_host(monkeypatch):
    ctx, gc = device_cache()
    del ctx.calls[:]

    def no_parse(*a):
        raise AssertionError("parse_annotation on the host")
    monkeypatch.setattr("pas_amd.gas_cache.parse_annotation", no_parse)
    gc.add_pod(pod("p1", "card0,card2", containers=((2, 100),)))
    gc.add_pod(pod("p2", "card0|", node="node-b", containers=((1, 1), (0, 0))))
    gc.add_pod(pod("p3", "card0", containers=((1, 1), (1, 1))))        # 1 segment, 2 containers
    gc.add_pod(pod("p4", "card0", node=""))                            # no node name
    gc.add_pod(pod("p5", "card0", node="elsewhere"))                   # a node never held
    gc.add_pod(pod("p6", ""))                                          # no card listed
    gc.add_pod(pod("p7", "nosuchcard"))                                # reaches the walker
    assert gc.flush() == [
        ("default&p1", POD_ADDED, OK), ("default&p2", POD_ADDED, OK),
        ("default&p3", POD_ADDED, BAD_ARGS), ("default&p4", POD_ADDED, BAD_ARGS),
        ("default&p5", POD_ADDED, OK), ("default&p6", POD_ADDED, OK),
        ("default&p7", POD_ADDED, OK)]
    assert ctx.calls == [("apply_names", 100, 101, [ADD] * 7,
                          ["node-a", "node-b", "node-a", "", "elsewhere", "node-a", "node-a"],
                          ["card0,card2", "card0|", "card0", "card0", "card0", "", "nosuchcard"],
                          [1, 2, 2, 1, 1, 1, 1])]
    assert gc.gen == 101
    assert set(gc.annotated) == {f"default&p{i}" for i in (1, 2, 5, 6, 7)}


def test_bookkeeping_skipped_delete_quirk_repeated_key_and_bind_echo():
    ctx, gc = device_cache(script={(1, 0): _lib.PAS_GAS_ERR_INPUT})
    del ctx.calls[:]
    bound = pod("mine", "card1")
    gc.note_bind(bound, "card1")
    gc.update_pod(None, bound)                                  # the informer's echo: skipped
    gc.add_pod(pod("p1", "card0"))
    gc.add_pod(pod("p1", "card0"))                              # repeated key: cuts the batch
    gc.update_pod(None, pod("gone", "card0", phase="Succeeded"))  # never added: skipped
    assert gc.flush() == [
        ("default&mine", POD_UPDATED, SKIPPED), ("default&p1", POD_ADDED, OK),
        ("default&p1", POD_ADDED, SKIPPED), ("default&gone", POD_COMPLETED, SKIPPED)]
    assert [c[0] for c in ctx.calls] == ["apply_names"] and ctx.calls[0][3] == [ADD]
    # a failed add leaves the key out, so the same pod is tried again, in a batch of its own
    gc.add_pod(pod("p2", "card0"))
    gc.add_pod(pod("p2", "card0"))
    assert gc.flush() == [("default&p2", POD_ADDED, ERR_INPUT), ("default&p2", POD_ADDED, OK)]
    assert [c[0] for c in ctx.calls] == ["apply_names"] * 3
    assert [c[1:3] for c in ctx.calls] == [(100, 101), (101, 102), (102, 103)]
    # podDeleted carries no annotation: one container is a no-op that forgets the key, two
    # containers are errBadArgs and the key stays; only podCompleted releases
    gc.add_pod(pod("two", "card0|card1", containers=((1, 1), (1, 1))))
    gc.flush()
    gc.delete_pod(pod("p1", "card0"))
    gc.delete_pod(pod("two", "card0|card1", containers=((1, 1), (1, 1))))
    gc.update_pod(None, pod("mine", "card1", phase="Failed"))
    assert gc.flush() == [("default&p1", POD_DELETED, OK), ("default&two", POD_DELETED, BAD_ARGS),
                          ("default&mine", POD_COMPLETED, OK)]
    assert ctx.calls[-1][3:6] == ([REMOVE, REMOVE, REMOVE], ["node-a"] * 3, ["", "", "card1"])
    assert set(gc.annotated) == {"default&p2", "default&two"}


def test_node_items_update_rows_grow_and_assign_slots():
    ctx, gc = device_cache()
    del ctx.calls[:]
    gc.add_pod(pod_obj("p1", "node-a", [(1, 100)], "card2"))
    gc.update_node(None, node_obj("node-a", ["card1", "card2"]))   # card0 leaves: parked
    gc.add_node(node_obj("node-c", ["card0", "card1"]))            # takes the spare slot
    gc.update_node(None, node_obj("node-a", ["card0", "card2"]))   # node-a again, same batch
    gc.add_pod(pod_obj("p2", "node-c", [(1, 100)], "card1"))
    gc.add_node(node_obj("node-d", ["card0"]))                     # no spare slot: 3 -> 67
    gc.update_node(None, node_obj("node-d", [f"card{i}" for i in range(5)]))  # 5 > 4: 8 slots
    results = gc.flush()
    assert [r[2] for r in results] == [OK] * 7
    assert [c[0] for c in ctx.calls] == [
        "apply_names",
        "names_assign", "nodes", "cards_update",                   # the first node batch
        "apply_names",
        "resize", "cards_resize", "names_resize", "names_assign", "nodes", "cards_update",
        "resize", "cards_resize", "names_resize", "nodes", "cards_update"]
    assert ctx.calls[1] == ("names_assign", ["node-c"], [2])       # the slot _plan_node chose
    assert ctx.calls[3] == ("cards_update", [0, 2, 0], [           # rows as each update left them
        ["card1", "card2", "card0", ""], ["card0", "card1", "", ""],
        ["card0", "card2", "card1", ""]])
    assert ctx.calls[5:9] == [("resize", 103, 104, 67, 4), ("cards_resize", 67, 4),
                              ("names_resize", 67), ("names_assign", ["node-d"], [3])]
    assert ctx.calls[11:14] == [("resize", 105, 106, 67, 8), ("cards_resize", 67, 8),
                                ("names_resize", 67)]
    assert ctx.calls[15] == ("cards_update", [3], [[f"card{i}" for i in range(5)] + [""] * 3])
    # the stub's tables are the cache's
    assert ctx.node_names[:4] == ["node-a", "node-b", "node-c", "node-d"]
    for slot in range(4):
        row = gc.card_names[slot] + gc.parked[slot]
        assert ctx.rows[slot] == row + [""] * (8 - len(row))


def test_compact_remaps_both_tables_and_rebuild_resends_cleared_rows():
    ctx, gc = device_cache()
    gc.update_node(None, node_obj("node-a", ["card1"]))            # card0, card2 parked
    gc.delete_node(node_obj("node-b", None))                       # idle: compact drops it
    gc.flush()
    del ctx.calls[:]
    src = gc.compact(spare_nodes=2)
    assert src == [0, -1, -1]
    assert [c[0] for c in ctx.calls] == ["compact", "cards_remap", "names_remap"]
    assert ctx.calls[1] == ("cards_remap", src) and ctx.calls[2] == ("names_remap", src)
    assert ctx.node_names == ["node-a", "", ""] and gc.node_names == ["node-a", None, None]
    assert ctx.rows[0] == ["card1", "card0", "card2", ""]
    del ctx.calls[:]
    gc.rebuild([pod_obj("p", "node-a", [(1, 1)], "card1")])
    assert [c[0] for c in ctx.calls] == ["set", "cards_update", "apply_names"]
    assert ctx.calls[1] == ("cards_update", [0], [["card1", "", "", ""]])  # the parked names go
    assert gc.parked == [[], [], []]


def test_both_modes_give_the_same_outcomes_over_the_stub():
    """One script through both modes: outcomes, annotated, card_names and parked agree item by
    item (the stub answers the walker's events with OK in both)."""
    class Plain(StubCtx):
        def gas_apply(self, gen_from, gen_to, kinds, *a):
            self.calls.append(("apply",))
            return np.zeros(len(kinds), np.int32)

    def script(gc):
        out = []
        gc.add_pod(pod_obj("a", "node-a", [(1, 1)], "card0,card1"))
        gc.add_pod(pod_obj("b", "node-b", [(1, 1), (1, 1)], "card0"))      # bad args
        gc.add_pod(pod_obj("c", "ghost", [(1, 1)], "card0"))               # unknown node
        gc.add_pod(pod_obj("a", "node-a", [(1, 1)], "card0,card1"))        # skipped
        out += gc.flush()
        gc.update_node(None, node_obj("node-a", ["card2", "card9"]))
        gc.add_node(node_obj("ghost", ["card0"]))
        gc.update_pod(None, pod_obj("a", "node-a", [(1, 1)], "card0,card1", phase="Failed"))
        gc.delete_pod(pod_obj("c", "ghost", [(1, 1)], "card0"))
        gc.delete_pod(pod_obj("b", "node-b", [(1, 1), (1, 1)], "card0"))   # never annotated
        out += gc.flush()
        return out, dict(gc.annotated), [list(c) for c in gc.card_names], gc.parked

    plain = Plain((3, 4, Q))
    plain.n_cards = N_CARDS.copy()
    default = GasCache(plain, 100, NAMES, [list(c) for c in CARDS], KINDS, n_cards=N_CARDS,
                       cap=CAP)
    _, device = device_cache()
    assert script(default) == script(device)
