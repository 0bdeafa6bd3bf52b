"""GasCache: the reference cache's pod event path over the device-resident GAS usage.

The reference's Cache (gpu-aware-scheduling/pkg/gpuscheduler/node_resource_cache.go) learns
about pods from an informer: addPodToCache / updatePodInCache / deletePodFromCache (:305-400)
queue work items, and handlePod (:493-538) turns each into adjustPodResources(add / remove)
straight from the pod's "gas-container-cards" annotation, keyed by its annotatedPods set.  That
is how the usage stays true when pods are bound by another extender replica, by an earlier run,
or are met in the informer's initial list.  Here the same decisions are made on the host and
the arithmetic runs on the device: events queue up and flush() sends them as ordered
pas_gas_apply batches, so the usage never leaves the device.
"""
import json
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .snapshot import (card_remap, gas_node_row, pack_card_names, pack_names, pack_node_strings,
                       parse_annotation)

CARD_ANNOTATION = "gas-container-cards"  # cardAnnotationName (scheduler.go)

POD_ADDED, POD_UPDATED, POD_COMPLETED, POD_DELETED = "added", "updated", "completed", "deleted"
NODE_ADDED, NODE_UPDATED, NODE_DELETED = "node_added", "node_updated", "node_deleted"
_NODE_ACTIONS = (NODE_ADDED, NODE_UPDATED, NODE_DELETED)
CARD_TIERS = (8, 16, _lib.PAS_GAS_MAX_CARDS)  # the kernels' max_cards tiers

# outcomes of one work item (handlePod's err, or why nothing was adjusted)
OK = "ok"                # adjustPodResources succeeded (annotatedPods changed)
SKIPPED = "skipped"      # "annotation already present" / "annotation already gone"
BAD_ARGS = "bad_args"    # errBadArgs: segment count != container count, or no node name
ERR_INPUT = "input"      # errInput (PAS_GAS_ERR_INPUT)
ERR_OVERFLOW = "overflow"  # errOverflow (PAS_GAS_ERR_OVERFLOW)
_STATUS = {_lib.PAS_GAS_OK: OK, _lib.PAS_GAS_ERR_INPUT: ERR_INPUT,
           _lib.PAS_GAS_ERR_OVERFLOW: ERR_OVERFLOW, _lib.PAS_GAS_ERR_BAD_ARGS: BAD_ARGS}


def pod_key(pod: dict) -> str:
    """getKey (node_resource_cache.go:451-453): namespace & name."""
    meta = pod.get("metadata") or {}
    return (meta.get("namespace") or "") + "&" + (meta.get("name") or "")


def is_completed_pod(pod: dict) -> bool:
    """isCompletedPod (utils.go:52-71): a deletion timestamp, or phase Failed / Succeeded."""
    if (pod.get("metadata") or {}).get("deletionTimestamp") is not None:
        return True
    return (pod.get("status") or {}).get("phase") in ("Failed", "Succeeded")


def _annotation_of(pod: dict) -> Optional[str]:
    return ((pod.get("metadata") or {}).get("annotations") or {}).get(CARD_ANNOTATION)


def _node_name(node: dict) -> str:
    return (node.get("metadata") or {}).get("name") or ""


def _node_dict(node: dict) -> dict:
    """A v1.Node object as snapshot.gas_node_row reads a node."""
    return {"labels": (node.get("metadata") or {}).get("labels") or {},
            "allocatable": (node.get("status") or {}).get("allocatable") or {}}


def _tier(cards: int) -> int:
    """The smallest max_cards tier that holds `cards` label cards."""
    for t in CARD_TIERS:
        if cards <= t:
            return t
    raise _lib.PasError(_lib.PAS_ECAPACITY,
                        f"{cards} cards > {_lib.PAS_GAS_MAX_CARDS} (PAS_GAS_MAX_CARDS)")


class GasCache:
    """The event path of the reference's Cache over a context's resident GAS snapshot.

    `ctx` holds the snapshot of generation `gen` built by snapshot.gas_snapshot_from_nodes over
    `node_names` with `card_names` and `kinds`; n_cards / cap are that snapshot's (rebuild
    uploads them again with zero usage).  Pods are v1.Pod JSON objects.  `requests(pod)`
    returns (req [C][Q] int64, req_mask [C] uint32, n_containers), containerRequests
    (utils.go:14-32); the default decodes the pod through pas_decode_pod_requests.

    add_pod / update_pod / delete_pod are the informer's handlers: they only queue.  flush()
    handles the queue in order as handlePod does and returns [(key, action, outcome)] per
    item.  Every decision reads annotatedPods as it stands when the item is handled, and
    annotatedPods changes only when the adjustment succeeded, so one pas_gas_apply batch
    holds at most one event per pod key: a second item for a key closes the batch, and its
    decision is made once the first batch's statuses are known.  deletePodFromCache's own
    look at annotatedPods (:384-391, taken when the informer calls, whatever the worker has
    handled by then) is made at the same point, as if the worker had caught up.

    A segment count that differs from the container count (or an empty node name) is
    errBadArgs (:192-196): answered here, nothing is sent.  An annotation without cards adjusts
    nothing and succeeds without a device call.  A node the snapshot does not hold has no
    usage to adjust: the item succeeds without a device call, where the reference would keep
    usage that no fit reads.

    The podDeleted quirk is reproduced as it is: the reference's podDeleted item carries no
    annotation (:393-399), so handlePod removes "".  strings.Split("", "|") is one empty
    segment: a pod with one container gets a no-op and its key is forgotten; a pod with
    several containers gets errBadArgs and its key stays.  Only podCompleted (an update of a
    pod that isCompletedPod) releases usage.

    note_bind(pod, annotation) records a pod this process bound itself: bindNode's
    adjustPodResources(add) sets annotatedPods too, so the informer's later update for that
    pod is skipped instead of being added twice.

    Node events.  add_node / update_node / delete_node take v1.Node JSON objects
    (metadata.name, metadata.labels, status.allocatable) and queue into the same queue, and
    flush() keeps the informer's order: a node item closes the open pod batch, consecutive
    node items go out as one pas_gas_nodes_update batch (one node may repeat in it), and pod
    items after a node item compute their card ranks from the card names as of that point.
    A node item reports (name, action, OK) or "dropped: card, ..." for parked cards lost.

    Slots are stable.  node_names[slot] is the slot's name, None for a spare slot
    (n_cards -1).  card_names[slot] lists the label cards in rank order and parked[slot] the
    parked cards behind them (snapshot.card_remap): a card that leaves the label keeps its
    usage in a parked slot and has it again when the label lists it again, as the reference's
    nodeStatuses keeps it by card name.  A deleted node keeps its slot and name with n_cards
    -1 and every card parked, so its usage is there when the name returns; a new name takes a
    spare slot.  compact() drops the spare slots and the deleted nodes without usage; nothing
    calls it implicitly.  The snapshot grows on the device (pas_gas_snapshot_resize) when no spare slot
    is left, by max(64, N / 8) slots rounded up to 64, and when a label lists more cards than
    max_cards, to the next of 8 / 16 / 64; parking never grows it.  card_names is changed in
    place (a GASExtender sharing the list sees the changes; GASExtender.nodes_changed takes
    the new node_names).

    device_events=True leaves the string work of a pod event to the device, as handlePod gets
    it: construction installs the context's card-name table (pas_gas_card_names_set: row slot =
    card_names[slot] + parked[slot]) and its node-name table (pas_names_set, spare slots as
    empty names; a node named "" is a ValueError, as in TasCache), and a pod batch is one
    pas_gas_apply_annotations_names call over the events' node names and annotation strings.
    The host keeps the annotatedPods decision and requests(pod) and nothing else: no split, no
    node lookup, no card lookup, and errBadArgs, the unknown node and the annotation without
    cards are answered by the device in the same batch (so every item that is not skipped
    takes part in the one-event-per-key rule).  Node items send their rows to the card-name
    table beside pas_gas_nodes_update, a first-seen node takes its slot through
    pas_names_assign (the lowest spare slot, which is the slot chosen here), and growth,
    compact and rebuild keep both tables in step.  Outcomes, annotated, card_names, parked and
    the resident usage are those of the default mode.  max_cards names the snapshot's card
    slots per node when the context cannot tell (from_nodes passes it).

    device_nodes=True (with device_events) leaves the string work of a node event to the device
    as well: a node batch is one pas_gas_nodes_update_strings_names call over the nodes' names,
    cards labels and allocatable literals as the informer hands them over
    (snapshot.pack_node_strings: nothing is split, sorted, parsed or looked up on the host).  The
    batch closes when a node name repeats, the rule pod batches follow per key.  First-seen names
    take their slots through pas_names_assign before the call (PAS_ECAPACITY there grows the
    node slots), and afterwards card_names[slot] and parked[slot] of the touched slots are read
    back with pas_gas_card_names_get_rows, n_cards and cap come from the call's outputs, and
    "dropped: ..." is the old host row minus the row read back, in old order.  PAS_ECAPACITY of
    the strings call changed nothing: a batch of several items is sent again in two halves, a
    single item grows the card slots to the tier its label needs and is sent again, so every
    item meets the max_cards the default mode gives it.  Outcomes, card_names, parked and the
    resident state equal the default mode's but for one case: a parked card named "" is an
    unused slot to the device (pas.h), so a card "" that leaves the label is parked once and
    forgotten by the next label update of its node, with its usage.
    from_nodes(..., device_nodes=True) is the cold start: an empty snapshot of the smallest
    tier and empty tables, then the nodes as one batch."""

    def __init__(self, ctx, gen: int, node_names: Sequence[str],
                 card_names: Sequence[Sequence[str]], kinds: Sequence[str],
                 n_cards=None, cap=None,
                 requests: Optional[Callable[[dict], Tuple[np.ndarray, np.ndarray, int]]] = None,
                 device_events: bool = False, max_cards: Optional[int] = None,
                 device_nodes: bool = False):
        if device_nodes and not device_events:
            raise ValueError("device_nodes needs device_events: the tables are installed by it")
        if device_events and "" in node_names:
            raise ValueError("device_events: the empty node name marks a spare slot")
        self.ctx, self.gen = ctx, gen
        self.node_names: List[Optional[str]] = list(node_names)
        self.node_index = {n: i for i, n in enumerate(node_names) if n is not None}
        self.card_names = card_names
        self.parked: List[List[str]] = [[] for _ in self.node_names]
        self.max_cards: Optional[int] = max_cards  # None: resolved by the first use (_k)
        self.kinds = list(kinds)
        self.n_cards, self.cap = n_cards, cap
        self._rows_owned = False  # n_cards / cap are copies this cache may write
        self._requests = requests if requests is not None else self._decode_requests
        self.annotated: Dict[str, str] = {}  # annotatedPods
        self._queue: List[Tuple[str, dict, str]] = []  # (action, pod or node, annotation)
        self.device_events = bool(device_events)
        self.device_nodes = bool(device_nodes)
        if self.device_events:
            k = self._k()
            ctx.gas_card_names_set(len(self.node_names), k,
                                   *pack_card_names(self.card_names, self.parked, k))
            ctx.names_set(*pack_names(self.node_names))

    @classmethod
    def from_nodes(cls, ctx, gen: int, nodes: Sequence[dict], kinds: Sequence[str],
                   spare_nodes: int = 0, **kw) -> "GasCache":
        """A cache over a fresh snapshot of the v1.Node objects `nodes` (zero usage) plus
        spare_nodes spare slots, uploaded as generation gen; max_cards is the smallest of
        8 / 16 / 64 that holds the largest label."""
        if kw.get("device_nodes"):  # nothing is read on the host: the nodes are the first batch
            n, k = len(nodes) + int(spare_nodes), CARD_TIERS[0]
            n_cards, cap = np.full(n, -1, np.int32), np.zeros((n, len(kinds)), np.int64)
            ctx.gas_snapshot_set(gen, n_cards, cap, np.zeros((n, k, len(kinds)), np.int64))
            cache = cls(ctx, gen, [None] * n, [[] for _ in range(n)], kinds, n_cards=n_cards,
                        cap=cap, max_cards=k, **kw)
            names = [_node_name(node) for node in nodes]
            if "" in names:
                raise ValueError("device_events: the empty node name marks a spare slot")
            if len(set(names)) == len(names):  # one batch, past the queue and its result list
                if nodes:
                    cache._send_node_strings([(name, NODE_ADDED, node)
                                              for name, node in zip(names, nodes)])
            else:
                for node in nodes:
                    cache.add_node(node)
                cache.flush()
            return cache
        rows = [gas_node_row(_node_dict(node), kinds) for node in nodes]
        names: List[Optional[str]] = [_node_name(node) for node in nodes]
        n, q = len(rows) + int(spare_nodes), len(kinds)
        k = _tier(max([1] + [len(cards) for _, _, cards in rows]))
        n_cards = np.full(n, -1, np.int32)
        cap = np.zeros((n, q), np.int64)
        for i, (nc, c, _) in enumerate(rows):
            n_cards[i], cap[i] = nc, c
        card_names = [cards for _, _, cards in rows] + [[] for _ in range(int(spare_nodes))]
        ctx.gas_snapshot_set(gen, n_cards, cap, np.zeros((n, k, q), np.int64))
        return cls(ctx, gen, names + [None] * int(spare_nodes), card_names, kinds,
                   n_cards=n_cards, cap=cap, max_cards=k, **kw)

    def _decode_requests(self, pod: dict):
        from . import wire
        req, mask, ncont, _ = wire.decode_pod_requests(json.dumps(pod).encode(), self.kinds)
        return req[0], mask[0], int(ncont[0])

    # ------------------------------------------------------------ informer handlers
    def add_pod(self, pod: dict):
        """addPodToCache (:305-327): a pod without the annotation waits for its update."""
        annotation = _annotation_of(pod)
        if annotation is not None:
            self._queue.append((POD_ADDED, pod, annotation))

    def update_pod(self, old_pod: Optional[dict], new_pod: dict):
        """updatePodInCache (:329-357): podUpdated, or podCompleted for a completed pod."""
        annotation = _annotation_of(new_pod)
        if annotation is not None:
            action = POD_COMPLETED if is_completed_pod(new_pod) else POD_UPDATED
            self._queue.append((action, new_pod, annotation))

    def delete_pod(self, pod: dict):
        """deletePodFromCache (:359-400): the item carries no annotation."""
        self._queue.append((POD_DELETED, pod, ""))

    def note_bind(self, pod: dict, annotation: str):
        """A bind of this process (pas_gas_bind* / pas_gas_place*) already committed the
        pod's usage: adjustPodResources(add) in bindNode sets annotatedPods[key]."""
        self.annotated[pod_key(pod)] = annotation

    def _queue_node(self, action: str, node: dict):
        if self.device_events and _node_name(node) == "":
            raise ValueError("device_events: the empty node name marks a spare slot")
        self._queue.append((action, node, ""))

    def add_node(self, node: dict):
        """A node the lister now knows (or knows again)."""
        self._queue_node(NODE_ADDED, node)

    def update_node(self, old_node: Optional[dict], new_node: dict):
        """A changed node: its cards label or its allocatable."""
        self._queue_node(NODE_UPDATED, new_node)

    def delete_node(self, node: dict):
        """A node the lister no longer knows: every fit on it is the FetchNode error."""
        self._queue_node(NODE_DELETED, node)

    # ------------------------------------------------------------ node items
    def _k(self) -> int:
        """max_cards of the resident snapshot."""
        if self.max_cards is None:
            shape = getattr(self.ctx, "gas_shape", None)
            self.max_cards = int(shape[1]) if shape and shape[1] else \
                max([1] + [len(c) for c in self.card_names])
        return self.max_cards

    def _grow(self, n_nodes: int, max_cards: int):
        """pas_gas_snapshot_resize, and the host tables with it."""
        self.ctx.gas_snapshot_resize(self.gen, self.gen + 1, n_nodes, max_cards)
        self.gen += 1
        if self.device_events:
            self.ctx.gas_card_names_resize(n_nodes, max_cards)
            self.ctx.names_resize(n_nodes)
        extra = n_nodes - len(self.node_names)
        self.node_names.extend([None] * extra)
        self.card_names.extend([] for _ in range(extra))  # in place: the extender shares it
        self.parked.extend([] for _ in range(extra))
        if self.n_cards is not None and self.cap is not None:
            self.n_cards = np.concatenate([np.asarray(self.n_cards, np.int32),
                                           np.full(extra, -1, np.int32)])
            cap = np.asarray(self.cap, np.int64)
            self.cap = np.concatenate([cap, np.zeros((extra, cap.shape[1]), np.int64)])
            self._rows_owned = True
        self.max_cards = max_cards

    def _plan_node(self, action: str, node: dict, send_pending):
        """One node item on the host tables: (outcome, update) with update = (slot, n_cards,
        cap [Q], src [max_cards], the row's card names) or None when nothing is sent.
        send_pending() sends the node updates planned so far; it runs before the snapshot has
        to grow."""
        name = _node_name(node)
        slot = self.node_index.get(name)
        if action == NODE_DELETED:
            if slot is None:
                return OK, None  # a node the snapshot never held
            n_cards, cap, cards = -1, np.zeros(len(self.kinds), np.int64), []
        else:
            n_cards, cap, cards = gas_node_row(_node_dict(node), self.kinds)
        k, n = self._k(), len(self.node_names)
        spare = None
        if slot is None:
            spare = next((i for i, nm in enumerate(self.node_names) if nm is None), None)
        grow_n = slot is None and spare is None
        if grow_n or len(cards) > k:
            send_pending()
            if grow_n:
                spare = n
                n += (max(64, n // 8) + 63) // 64 * 64
            self._grow(n, _tier(len(cards)) if len(cards) > k else k)
            k = self.max_cards
        if slot is None:
            slot = spare
            self.node_names[slot] = name
            self.node_index[name] = slot
            if self.device_events:  # the name table's rule is this one: the lowest spare slot
                _, _, new_slot = self.ctx.names_assign(*pack_names([name]), 1, want_slots=False)
                assert list(new_slot) == [slot], (name, slot, list(new_slot))
        old_slots = list(self.card_names[slot]) + self.parked[slot]
        if action == NODE_DELETED:  # the row stays where it is, every card parked
            src, slots, dropped = list(range(k)), old_slots, []
        else:
            src, slots, dropped = card_remap(old_slots, cards, k)
        self.card_names[slot] = slots[:len(cards)]
        self.parked[slot] = slots[len(cards):]
        if self.n_cards is not None and self.cap is not None:
            if not self._rows_owned:  # the caller's arrays stay as they are
                self.n_cards = np.array(self.n_cards, np.int32)
                self.cap = np.array(self.cap, np.int64)
                self._rows_owned = True
            self.n_cards[slot], self.cap[slot] = n_cards, cap
        outcome = OK if not dropped else "dropped: " + ", ".join(dropped)
        return outcome, (slot, n_cards, cap, src, list(slots))

    def _send_nodes(self, updates) -> List[int]:
        """One pas_gas_nodes_update call for the planned updates, in order (device_events: and
        one pas_gas_card_names_update with the rows' names as each update left them)."""
        st = self.ctx.gas_nodes_update(self.gen, self.gen + 1, [u[0] for u in updates],
                                       [u[1] for u in updates],
                                       np.array([u[2] for u in updates], np.int64),
                                       np.array([u[3] for u in updates], np.int32))
        self.gen += 1
        if self.device_events:
            self.ctx.gas_card_names_update(
                [u[0] for u in updates],
                *pack_card_names([u[4] for u in updates], None, self._k()))
        return [int(s) for s in st]

    def _own_rows(self):
        if self.n_cards is not None and self.cap is not None and not self._rows_owned:
            self.n_cards = np.array(self.n_cards, np.int32)  # the caller's arrays stay
            self.cap = np.array(self.cap, np.int64)
            self._rows_owned = True

    def _send_node_strings(self, items) -> List[str]:
        """device_nodes: the outcomes of one batch of node items (name, action, node), no name
        twice, as one pas_gas_nodes_update_strings_names call (two halves, or a larger tier, on
        PAS_ECAPACITY)."""
        names = [name for name, _, _ in items]
        live = [name for name, action, _ in items if action != NODE_DELETED]
        slot_of: Dict[str, int] = {}
        while live:  # first-seen names take the lowest spare slots, in order
            try:
                slots, _, _ = self.ctx.names_assign(*pack_names(live))
                slot_of.update(zip(live, slots.tolist()))
                for name, slot in slot_of.items():
                    if self.node_names[slot] is None:
                        self.node_names[slot] = name
                        self.node_index[name] = slot
                break
            except _lib.PasError as e:
                if e.code != _lib.PAS_ECAPACITY:
                    raise
                n = len(self.node_names)
                self._grow(n + (max(64, n // 8) + 63) // 64 * 64, self._k())
        gone = [name for name, action, _ in items if action == NODE_DELETED]
        if gone:
            slot_of.update(zip(gone, self.ctx.names_resolve(*pack_names(gone)).tolist()))
        packed = pack_node_strings(
            [None if action == NODE_DELETED else _node_dict(node) for _, action, node in items],
            self.kinds)
        try:
            st, n_cards, cap, _ = self.ctx.gas_nodes_update_strings_names(
                self.gen, self.gen + 1, *pack_names(names), *packed)
        except _lib.PasError as e:
            if e.code != _lib.PAS_ECAPACITY:
                raise
            if len(items) > 1:  # nothing has changed: the items before the large label go first
                half = len(items) // 2
                return (self._send_node_strings(items[:half]) +
                        self._send_node_strings(items[half:]))
            self._grow(len(self.node_names), _tier(int(e.need_cards)))
            return self._send_node_strings(items)
        self.gen += 1
        st, labels = st.tolist(), np.maximum(n_cards, 0).tolist()
        outcomes = [OK if s == _lib.PAS_GAS_OK else ERR_INPUT for s in st]
        touched = [(u, slot_of[name]) for u, name in enumerate(names)
                   if st[u] == _lib.PAS_GAS_OK and slot_of[name] >= 0]
        if not touched:
            return outcomes
        at, slots = (list(x) for x in zip(*touched))
        rows = self.ctx.gas_card_names_get_rows(slots, decode=True)
        for u, slot, row in zip(at, slots, rows):
            label = labels[u]
            parked = [c for c in row[label:] if c]  # (a parked "" is an unused slot)
            old = self.card_names[slot] + self.parked[slot]
            self.card_names[slot], self.parked[slot] = row[:label], parked
            if old:
                new = set(row)
                dropped = [c for c in old if c and c not in new]
                if dropped:
                    outcomes[u] = "dropped: " + ", ".join(dropped)
        if self.n_cards is not None and self.cap is not None:
            self._own_rows()
            self.n_cards[slots], self.cap[slots] = n_cards[at], cap[at]
        return outcomes

    # ------------------------------------------------------------ the worker
    def _plan(self, action: str, pod: dict, annotation: str):
        """handlePod's switch and adjustPodResources' argument check for one item: an outcome
        answered on the host, or the device event (kind, node, req, mask, ncont, cpc, ranks)."""
        key = pod_key(pod)
        add = action in (POD_ADDED, POD_UPDATED)
        if add == (key in self.annotated):  # already present / already gone
            return SKIPPED
        req, mask, ncont = self._requests(pod)
        if self.device_events:  # handlePod's arguments as they are: the device does the rest
            kind = _lib.PAS_GAS_EV_ADD if add else _lib.PAS_GAS_EV_REMOVE
            return kind, (pod.get("spec") or {}).get("nodeName") or "", req, mask, ncont, annotation
        segments = annotation.split("|")
        node_name = (pod.get("spec") or {}).get("nodeName") or ""
        if len(segments) != ncont or node_name == "":
            return BAD_ARGS
        node = self.node_index.get(node_name)
        names = self.card_names[node] if node is not None else []
        cpc, ranks = parse_annotation(annotation, names)
        if node is None or not ranks:
            return OK
        kind = _lib.PAS_GAS_EV_ADD if add else _lib.PAS_GAS_EV_REMOVE
        return kind, node, req, mask, ncont, cpc, ranks

    def _settle(self, key: str, action: str, annotation: str, outcome: str):
        if outcome == OK:
            if action in (POD_ADDED, POD_UPDATED):
                self.annotated[key] = annotation
            else:
                self.annotated.pop(key, None)

    def _send(self, batch) -> List[int]:
        """One pas_gas_apply call for the batch's events, pod e = event e (device_events: one
        pas_gas_apply_annotations_names call over the node names and annotation strings)."""
        e = len(batch)
        q = len(self.kinds)
        c = max(1, max(ev[4] for ev in batch))
        req = np.zeros((e, c, q), np.int64)
        mask = np.zeros((e, c), np.uint32)
        ncont = np.zeros(e, np.int32)
        if self.device_events:
            for i, (_, _, r, m, nc, _) in enumerate(batch):
                ncont[i] = nc
                req[i, :nc] = np.asarray(r, np.int64).reshape(-1, q)[:nc]
                mask[i, :nc] = np.asarray(m, np.uint32)[:nc]
            st = self.ctx.gas_apply_annotations_names(
                self.gen, self.gen + 1, np.fromiter((ev[0] for ev in batch), np.int32, e),
                np.arange(e, dtype=np.int32), *pack_names([ev[1] for ev in batch]), req, mask,
                ncont, *pack_names([ev[5] for ev in batch]))
            self.gen += 1
            return [int(s) for s in st]
        ld = max(1, max(len(ev[6]) for ev in batch))
        cpc = np.zeros((e, c), np.int32)
        cards = np.full((e, ld), -1, np.int32)
        kinds = np.zeros(e, np.int32)
        nodes = np.zeros(e, np.int32)
        for i, (kind, node, r, m, nc, pc, ranks) in enumerate(batch):
            kinds[i], nodes[i], ncont[i] = kind, node, nc
            req[i, :nc] = np.asarray(r, np.int64).reshape(-1, q)[:nc]
            mask[i, :nc] = np.asarray(m, np.uint32)[:nc]
            cpc[i, :nc] = pc
            cards[i, :len(ranks)] = ranks
        st = self.ctx.gas_apply(self.gen, self.gen + 1, kinds, np.arange(e, dtype=np.int32),
                                nodes, req, mask, ncont, cpc, cards)
        self.gen += 1
        return [int(s) for s in st]

    def flush(self) -> List[Tuple[str, str, str]]:
        """Handle the queued items in order; [(key, action, outcome)] per item."""
        queue, self._queue = self._queue, []
        results: List[Optional[Tuple[str, str, str]]] = [None] * len(queue)
        batch, slots, keys = [], [], set()

        def close():
            if batch:
                for (i, key, action, annotation), s in zip(slots, self._send(batch)):
                    outcome = _STATUS.get(s, ERR_INPUT)
                    self._settle(key, action, annotation, outcome)
                    results[i] = (key, action, outcome)
            batch.clear()
            slots.clear()
            keys.clear()

        node_batch, node_slots = [], []  # planned node updates and their (i, name, action, outcome)

        def close_nodes():
            if node_batch:
                for (i, name, action, outcome), s in zip(node_slots, self._send_nodes(node_batch)):
                    results[i] = (name, action, outcome if s == _lib.PAS_GAS_OK else ERR_INPUT)
            node_batch.clear()
            node_slots.clear()

        string_batch, string_at = [], []  # device_nodes: (name, action, node) and their i
        string_names = set()

        def close_strings():
            if string_batch:
                for i, item, outcome in zip(string_at, string_batch,
                                            self._send_node_strings(string_batch)):
                    results[i] = (item[0], item[1], outcome)
            string_batch.clear()
            string_at.clear()
            string_names.clear()

        for i, (action, pod, annotation) in enumerate(queue):
            if action in _NODE_ACTIONS and self.device_nodes:
                close()  # a node item closes the open pod batch
                name = _node_name(pod)
                if name in string_names:
                    close_strings()  # its row is the one the first item leaves
                string_names.add(name)
                string_batch.append((name, action, pod))
                string_at.append(i)
                continue
            close_strings()
            if action in _NODE_ACTIONS:
                close()  # a node item closes the open pod batch
                outcome, update = self._plan_node(action, pod, close_nodes)
                if update is None:
                    results[i] = (_node_name(pod), action, outcome)
                else:
                    node_batch.append(update)
                    node_slots.append((i, _node_name(pod), action, outcome))
                continue
            close_nodes()  # the pod's ranks and its event follow the node updates
            key = pod_key(pod)
            if key in keys:  # its decision needs the first event's status
                close()
            plan = self._plan(action, pod, annotation)
            if isinstance(plan, str):
                self._settle(key, action, annotation, plan)
                results[i] = (key, action, plan)
                continue
            batch.append(plan)
            slots.append((i, key, action, annotation))
            keys.add(key)
        close()
        close_nodes()
        close_strings()
        return results  # type: ignore[return-value]

    def compact(self, spare_nodes: int = 0) -> List[int]:
        """Drop the dead node slots with one pas_gas_snapshot_compact call and return the map
        applied: new slot j is old slot map[j], or a spare slot for -1.

        The queue is flushed first (a caller that wants the items' outcomes calls flush()
        itself before).  Dead are the spare slots and the slots of deleted nodes (n_cards -1)
        whose usage, read back from the device, is zero in every card slot, label and parked.
        A deleted node that still holds usage keeps its slot and name, as the reference keeps
        its nodeStatuses entry by name (node_resource_cache.go:64,259-272).  The live slots
        keep their order and spare_nodes spare slots follow them; node_names, card_names (in
        place), parked and the n_cards / cap rows move with them.  A TasCache over the same
        slots applies the same map: src = gas.compact(); tas.compact(src); its metric entries
        of names that lost their slot are skipped_nodes from then on.
        GASExtender.nodes_changed takes the new node_names."""
        self.flush()
        _, n_cards, cap = self.ctx.gas_snapshot_get_nodes()
        _, used = self.ctx.gas_snapshot_get()
        idle = ~used.reshape(len(used), -1).any(axis=1)
        src = [i for i, name in enumerate(self.node_names)
               if name is not None and not (n_cards[i] == -1 and idle[i])]
        src += [-1] * int(spare_nodes)
        self.ctx.gas_snapshot_compact(self.gen, self.gen + 1, src)
        self.gen += 1
        if self.device_events:
            self.ctx.gas_card_names_remap(src)
            self.ctx.names_remap(src)
        self.node_names = [self.node_names[s] if s >= 0 else None for s in src]
        self.node_index = {n: i for i, n in enumerate(self.node_names) if n is not None}
        self.card_names[:] = [self.card_names[s] if s >= 0 else [] for s in src]
        self.parked = [self.parked[s] if s >= 0 else [] for s in src]
        if self.n_cards is not None and self.cap is not None:
            at = np.asarray(src, np.int64)
            self.n_cards = np.where(at >= 0, n_cards[at], -1).astype(np.int32)
            self.cap = np.where((at >= 0)[:, None], cap[at], 0).astype(np.int64)
            self._rows_owned = True
        return src

    def rebuild(self, pods: Sequence[dict]) -> List[Tuple[str, str, str]]:
        """The cold start: zero usage, then every annotated pod as the informer's initial
        list delivers it (addPodToCache each, so one ADD batch unless a key repeats)."""
        if self.n_cards is None or self.cap is None:
            raise ValueError("rebuild needs the snapshot's n_cards and cap")
        n_cards = np.ascontiguousarray(self.n_cards, np.int32)
        cap = np.ascontiguousarray(self.cap, np.int64)
        # the current slots: max_cards as node events left it (parked usage starts at zero too)
        k = self.max_cards if self.max_cards is not None else \
            max([1] + [len(c) for c in self.card_names])
        self.gen += 1
        self.ctx.gas_snapshot_set(self.gen, n_cards, cap,
                                  np.zeros((len(n_cards), k, len(self.kinds)), np.int64))
        if self.device_events:  # the rows whose parked names go
            rows = [s for s, p in enumerate(self.parked) if p]
            if rows:
                self.ctx.gas_card_names_update(
                    rows, *pack_card_names([self.card_names[s] for s in rows], None, k))
        self.parked = [[] for _ in self.node_names]
        self.annotated.clear()
        self._queue = []
        for pod in pods:
            self.add_pod(pod)
        return self.flush()
