"""GasCache(device_events=True, device_nodes=True) against a stub context (no GPU): the call plan
of a node batch (one strings call, the rows read back afterwards, nothing split, sorted, parsed or
looked up on the host), a batch cut at a repeated node, growth and resend on PAS_ECAPACITY, and
outcomes equal to the default mode's on a scripted trace.  The stub answers what the device would
by the rules of pas.h, so both modes can be driven side by side."""
import numpy as np
import pytest

from pas_amd import _lib, snapshot
from pas_amd.gas_cache import (ERR_INPUT, NODE_ADDED, NODE_DELETED, NODE_UPDATED, OK, GasCache)
from test_gas_cache_device_events import CAP, CARDS, N_CARDS, NAMES, StubCtx, unpack
from test_gas_cache_nodes import KINDS, Q, node_obj, pod_obj

GONE, NO_LABEL, LABEL = (_lib.PAS_GAS_NODE_GONE, _lib.PAS_GAS_NODE_NO_LABEL,
                         _lib.PAS_GAS_NODE_LABEL)


class StringsStub(StubCtx):
    """The stub of the device_events tests plus the node-strings verbs, modelled on the rules of
    pas_gas_nodes_update_strings: rule 5 on the stub's own rows."""

    def names_assign(self, off, blob, new_cap=None, want_slots=True):
        names = unpack(off, blob)
        new = [n for n in dict.fromkeys(names) if n not in self.node_names]
        if len(new) > self.node_names.count(""):
            self.calls.append(("names_assign_full", names))
            e = _lib.PasError(_lib.PAS_ECAPACITY, "no spare slot")
            e.n_new = len(new)
            raise e
        super().names_assign(off, blob)
        return (np.array([self.node_names.index(n) for n in names], np.int32),) + (None, None)

    def names_resolve(self, off, blob):
        names = unpack(off, blob)
        self.calls.append(("names_resolve", names))
        return np.array([self.node_names.index(n) if n in self.node_names else -1
                         for n in names], np.int32)

    def gas_nodes_update_strings_names(self, gen_from, gen_to, name_off, name_blob, states,
                                       label_off, label_blob, cap_off, cap_blob):
        names, labels = unpack(name_off, name_blob), unpack(label_off, label_blob)
        lits = unpack(cap_off, cap_blob)
        assert len(set(names)) == len(names), "a node twice in one batch"
        k, q = self.k, self.gas_shape[2]
        need = max([len(set(l.split("."))) for l, s in zip(labels, states) if s == LABEL] + [0])
        if need > k:
            self.calls.append(("strings_full", gen_from, names, need))
            e = _lib.PasError(_lib.PAS_ECAPACITY, "a label lists more cards")
            e.need_cards = min(need, 65)
            raise e
        st, n_cards, cap, dropped = [], [], np.zeros((len(names), q), np.int64), []
        for u, (name, state, label) in enumerate(zip(names, states, labels)):
            slot = self.node_names.index(name) if name in self.node_names else -1
            if name == "" or (slot < 0 and state != GONE):
                st.append(_lib.PAS_GAS_ERR_INPUT), n_cards.append(0), dropped.append(0)
                continue
            st.append(_lib.PAS_GAS_OK)
            dropped.append(0)
            if state != LABEL:
                n_cards.append(state)  # -1 / 0: the row stays
                if slot >= 0:
                    self.n_cards[slot] = state
                continue
            pieces = label.split(".")
            cards = snapshot.go_sort_strings(set(pieces))
            for j in range(q):
                lit = lits[u * q + j]
                value = snapshot.quantity_as_int64(lit) if lit else 0
                cap[u, j] = abs(value) // len(pieces) * (-1 if value < 0 else 1)
            old, n_old = self.rows[slot], max(int(self.n_cards[slot]), 0)
            parked = [c for j, c in enumerate(old)
                      if c not in cards and not (c == "" and j >= n_old)]
            keep = k - len(cards)
            dropped[-1] = len(parked[keep:])
            row = cards + parked[:keep]
            self.rows[slot] = row + [""] * (k - len(row))
            self.n_cards[slot] = len(cards)
            n_cards.append(len(cards))
        self.calls.append(("strings", gen_from, gen_to, names, [int(s) for s in states], labels,
                           lits))
        return (np.array(st, np.int32), np.array(n_cards, np.int32), cap,
                np.array(dropped, np.int32))

    def gas_card_names_get_rows(self, slots, decode=False):
        self.calls.append(("get_rows", [int(s) for s in slots]))
        assert decode, "the cache takes the names as str"
        return [list(self.rows[s]) for s in slots]

    def gas_nodes_update(self, *a):
        raise AssertionError("device_nodes sends no pre-parsed node batch")

    def gas_card_names_update(self, *a):
        raise AssertionError("device_nodes sends no host copy of the names")


def strings_cache():
    ctx = StringsStub((3, 4, Q))
    ctx.n_cards = N_CARDS.copy()
    gc = GasCache(ctx, 100, NAMES, [list(c) for c in CARDS], KINDS, n_cards=N_CARDS, cap=CAP,
                  device_events=True, device_nodes=True)
    del ctx.calls[:]
    return ctx, gc


def test_device_nodes_needs_the_tables():
    with pytest.raises(ValueError):
        GasCache(StringsStub((3, 4, Q)), 1, NAMES, [list(c) for c in CARDS], KINDS,
                 device_nodes=True)


def test_one_strings_call_per_batch_and_no_string_work_on_the_host(monkeypatch):
    ctx, gc = strings_cache()

    def banned(name):
        def f(*a, **kw):
            raise AssertionError(name + " on the host")
        return f
    for name in ("gas_node_row", "card_remap", "pack_card_names"):
        monkeypatch.setattr("pas_amd.gas_cache." + name, banned(name))

    class NoProbe(dict):
        def get(self, *a):
            raise AssertionError("node_index probed")
        __getitem__ = __contains__ = get
    gc.node_index = NoProbe(gc.node_index)
    node_a = node_obj("node-a", ["card2", "card1", "card2"])          # card0 leaves: parked
    node_a["status"]["allocatable"]["gpu.intel.com/other"] = "5"
    gc.update_node(None, node_a)
    gc.add_node(node_obj("node-c", ["card10", "card2", "card1"]))      # first seen: the spare slot
    gc.delete_node(node_obj("node-b", None))
    gc.delete_node(node_obj("ghost", None))                            # never held
    gc.update_node(None, node_obj("node-z", None))                     # no label, no slot left
    results = gc.flush()
    assert [c[0] for c in ctx.calls] == ["names_assign_full", "resize", "cards_resize",
                                         "names_resize", "names_assign", "names_resolve",
                                         "strings", "get_rows"]
    assert ctx.calls[1] == ("resize", 100, 101, 67, 4)
    assert ctx.calls[4][1:] == (["node-a", "node-c", "node-z"], [2, 3])
    assert ctx.calls[5] == ("names_resolve", ["node-b", "ghost"])
    assert ctx.calls[6] == (
        "strings", 101, 102, ["node-a", "node-c", "node-b", "ghost", "node-z"],
        [LABEL, LABEL, GONE, GONE, NO_LABEL], ["card2.card1.card2", "card10.card2.card1", "", "", ""],
        ["12", "12000", "12", "12000", "", "", "", "", "", ""])   # the literals as they are
    assert ctx.calls[7] == ("get_rows", [0, 2, 1, 3])
    assert results == [("node-a", NODE_UPDATED, OK), ("node-c", NODE_ADDED, OK),
                       ("node-b", NODE_DELETED, OK), ("ghost", NODE_DELETED, OK),
                       ("node-z", NODE_UPDATED, OK)]
    assert gc.gen == 102
    assert gc.card_names[:4] == [["card1", "card2"], [], ["card1", "card10", "card2"], []]
    assert gc.parked[:4] == [["card0"], ["card0"], [], []]
    assert gc.node_names[:4] == ["node-a", "node-b", "node-c", "node-z"]
    assert list(gc.n_cards[:4]) == [2, -1, 3, 0]
    assert gc.cap[0].tolist() == [4, 4000] and gc.cap[2].tolist() == [4, 4000]


def test_a_repeated_node_cuts_the_batch_and_pods_follow_the_nodes():
    ctx, gc = strings_cache()
    gc.update_node(None, node_obj("node-a", ["card1", "card2"]))
    gc.update_node(None, node_obj("node-b", ["card0", "card5"]))
    gc.update_node(None, node_obj("node-a", ["card0"]))                # node-a again: a new batch
    gc.add_pod(pod_obj("p", "node-a", [(1, 1)], "card0"))
    gc.update_node(None, node_obj("node-a", ["card0", "card1"]))
    assert [r[2] for r in gc.flush()] == [OK] * 5
    plan = [(c[0], c[3]) for c in ctx.calls if c[0] in ("strings", "apply_names")]
    assert plan == [("strings", ["node-a", "node-b"]), ("strings", ["node-a"]),
                    ("apply_names", [_lib.PAS_GAS_EV_ADD]), ("strings", ["node-a"])]
    assert [c[0] for c in ctx.calls].count("get_rows") == 3
    assert gc.card_names[0] == ["card0", "card1"] and gc.parked[0] == ["card2"]


def test_capacity_halves_the_batch_then_grows_a_tier_and_sends_again():
    ctx, gc = strings_cache()
    big = [f"card{i}" for i in range(9)]
    gc.update_node(None, node_obj("node-a", ["card1"]))                # card0, card2 parked at k = 4
    gc.update_node(None, node_obj("node-b", big))                      # 9 > 4: the 16 tier
    results = gc.flush()
    assert [c[0] for c in ctx.calls if c[0] != "names_assign"] == [
        "strings_full",                      # both: nothing changed
        "strings", "get_rows",               # node-a alone, at max_cards 4 as in the default mode
        "strings_full", "resize", "cards_resize", "names_resize", "strings", "get_rows"]
    assert ctx.calls[0] == ("names_assign", ["node-a", "node-b"], [])
    full = [c for c in ctx.calls if c[0] == "strings_full"]
    assert [c[2:] for c in full] == [(["node-a", "node-b"], 9), (["node-b"], 9)]
    assert ("resize", 101, 102, 3, 16) in ctx.calls and ("cards_resize", 3, 16) in ctx.calls
    assert results == [("node-a", NODE_UPDATED, OK), ("node-b", NODE_UPDATED, OK)]
    assert gc.max_cards == 16 and gc.card_names[1] == snapshot.go_sort_strings(big)
    # 65 distinct cards are past every tier
    gc.update_node(None, node_obj("node-a", [f"c{i}" for i in range(70)]))
    with pytest.raises(_lib.PasError) as e:
        gc.flush()
    assert e.value.code == _lib.PAS_ECAPACITY


def test_dropped_and_err_input_outcomes():
    ctx, gc = strings_cache()
    gc.update_node(None, node_obj("node-a", ["x0", "x1", "x2"]))       # card0..2 parked: 6 > 4
    assert gc.flush() == [("node-a", NODE_UPDATED, "dropped: card1, card2")]
    assert gc.card_names[0] == ["x0", "x1", "x2"] and gc.parked[0] == ["card0"]
    ctx.node_names[1] = "renamed"  # the device no longer knows node-b: its update is refused
    gc.update_node(None, node_obj("node-b", ["card0"]))
    ctx.names_assign = lambda off, blob, **kw: (np.array([-1], np.int32), None, None)
    assert gc.flush() == [("node-b", NODE_UPDATED, ERR_INPUT)]


def trace(gc):
    out = []
    gc.add_pod(pod_obj("a", "node-a", [(1, 1)], "card0,card1"))
    gc.update_node(None, node_obj("node-a", ["card2", "card9"]))       # card0, card1 parked
    gc.add_node(node_obj("node-c", ["card1", "card0", "card1"]))       # gpuCount 3, 2 cards
    gc.update_node(None, node_obj("node-b", None))                     # the label goes
    out += gc.flush()
    gc.update_node(None, node_obj("node-a", ["card0", "card3", "card4"]))  # 3 + 3 parked > 4
    gc.delete_node(node_obj("node-c", None))
    gc.delete_node(node_obj("nobody", None))
    gc.add_node(node_obj("node-d", ["card0"]))                         # grows the node slots
    gc.update_pod(None, pod_obj("a", "node-a", [(1, 1)], "card0,card1", phase="Failed"))
    gc.add_node(node_obj("node-c", ["card0"]))                         # a deleted node returns
    gc.update_node(None, node_obj("node-c", ["card0", "card1", "card7"]))
    gc.update_node(None, node_obj("node-d", [f"card{i}" for i in range(6)]))  # 6 > 4: 8 slots
    out += gc.flush()
    return (out, dict(gc.annotated), [list(c) for c in gc.card_names], gc.parked,
            list(gc.node_names), gc.n_cards.tolist(), gc.cap.tolist(), gc.max_cards)


def test_outcomes_equal_the_default_mode_on_a_scripted_trace():
    class Plain(StubCtx):
        def gas_apply(self, gen_from, gen_to, kinds, *a):
            return np.zeros(len(kinds), np.int32)

    plain = Plain((3, 4, Q))
    plain.n_cards = N_CARDS.copy()
    default = GasCache(plain, 100, NAMES, [list(c) for c in CARDS], KINDS, n_cards=N_CARDS,
                       cap=CAP)
    _, device = strings_cache()
    want, got = trace(default), trace(device)
    assert got == want
    assert any(r[2].startswith("dropped: ") for r in got[0])


def test_the_empty_card_rule_is_pinned():
    """A card "" that leaves the label is parked once and is an unused slot from then on: the
    next label update of its node forgets it, where the default mode keeps it parked."""
    _, gc = strings_cache()
    gc.update_node(None, node_obj("node-b", ["", "card0"]))
    gc.update_node(None, node_obj("node-b", ["card0"]))                # "" leaves the label
    assert [r[2] for r in gc.flush()] == [OK, OK]
    assert gc.card_names[1] == ["card0"] and gc.parked[1] == []        # no parked name ""
    gc.update_node(None, node_obj("node-b", ["card1", "card2", "card3", "card4"]))
    assert gc.flush() == [("node-b", NODE_UPDATED, "dropped: card0")]  # "" is not counted


def test_cold_start_is_one_batch():
    ctx = StringsStub((0, 0, Q))
    nodes = [node_obj(f"n{i}", [f"card{j}" for j in range(1 + i % 3)]) for i in range(5)]
    gc = GasCache.from_nodes(ctx, 5, nodes, KINDS, spare_nodes=1, device_events=True,
                             device_nodes=True)
    assert [c[0] for c in ctx.calls] == ["set", "cards_set", "names_set", "names_assign",
                                         "strings", "get_rows"]
    assert ctx.calls[0] == ("set", 5, (6, 8, Q)) and ctx.calls[4][3] == [f"n{i}" for i in range(5)]
    plain = StubCtx((0, 0, Q))
    want = GasCache.from_nodes(plain, 5, nodes, KINDS, spare_nodes=1)
    assert (gc.node_names, gc.card_names, gc.parked) == (want.node_names, want.card_names,
                                                         want.parked)
    assert np.array_equal(gc.n_cards, want.n_cards) and np.array_equal(gc.cap, want.cap)
    assert gc.max_cards == want.max_cards == 8


def test_pack_node_strings():
    nodes = [None, {"labels": {}, "allocatable": {KINDS[0]: "4"}},
             {"labels": {snapshot.GPU_LIST_LABEL: ""}, "allocatable": {KINDS[1]: "1Gi", "cpu": "2"}},
             {"labels": {snapshot.GPU_LIST_LABEL: "a.b"}, "allocatable": {KINDS[0]: "8"}}]
    states, l_off, l_blob, c_off, c_blob = snapshot.pack_node_strings(nodes, KINDS + ["cpu"])
    assert states.tolist() == [GONE, NO_LABEL, LABEL, LABEL]
    assert unpack(l_off, l_blob) == ["", "", "", "a.b"]
    # no literal of a gone or unlabelled node, none of a kind outside "gpu.intel.com/"
    assert unpack(c_off, c_blob) == ["", "", "", "", "", "", "", "1Gi", "", "8", "", ""]
