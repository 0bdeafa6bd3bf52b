"""Host-side snapshot builders: the reference's cache contents in the
layouts of pas_tas_snapshot_set / pas_gas_snapshot_set.  This is the work the Go shim does once
per cache refresh; it is restated here so the whole path can be exercised from the
reference's own data shapes (metric maps of Quantity strings, node labels, usage maps).

TAS (cache/autoupdating.go:76-85, metrics/client.go:25-32): one column per metric name, one
row bit per node that has the metric, value * 10^scale exact (pas_quantity_to_scaled) with the
column's scale the most decimal places among its values (at least 3, milli): ParseQuantity
keeps at most 9, so every column is exact unless its range at that scale passes int64
(pas_tas_snapshot_set_scale).

GAS (gpuscheduler/scheduler.go:132-178, 269-275; node_resource_cache.go:474-491):
  cards      strings.Split(label "gpu.intel.com/cards", ".") -- duplicates and empty names
             included -- gives gpuCount; the cards a selection walks are the node's usage map
             keys plus the label cards (addEmptyResourceMaps), in sort.Strings order, minus
             cards not in the label (skipped as "vanished"): the sorted distinct label cards
  capacity   AsInt64 of every allocatable "gpu.intel.com/*" resource, divided by gpuCount
             (truncating); a kind the node does not advertise has capacity 0 (fails as missing)
  used       the usage map of each of those cards (a missing kind is 0)
  n_cards    number of those cards; 0 without the label (errWontFit, :290-298); -1 for a node
             the lister does not know (FetchNode error, :282-288)
"""
from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .context import (quantity_as_int64, quantity_decimals, quantity_to_scaled,
                      quantity_to_wide, w64)

GPU_LIST_LABEL = "gpu.intel.com/cards"
RESOURCE_PREFIX = "gpu.intel.com/"


def tas_snapshot_from_metrics(metrics: Mapping[str, Mapping[str, str]],
                              node_names: Sequence[str],
                              metric_names: Optional[Sequence[str]] = None):
    """(v [M][N] int64, present [M][W64] uint64, scale [M] int32) from {metric: {node:
    quantity string}}: column m holds value * 10^scale[m] exactly, scale[m] the most decimal
    places among the column's values (pas_quantity_decimals; 3 for a column of milli-exact
    values or none), for Context.tas_snapshot_set(gen, v, present, scale).  Nodes not in
    node_names are ignored.  A column whose values need more range than int64 at that scale
    raises PasError(PAS_ENOTEXACT) naming the metric: no value is dropped."""
    metric_names = list(metrics) if metric_names is None else list(metric_names)
    index = {n: i for i, n in enumerate(node_names)}
    n, m = len(node_names), len(metric_names)
    v = np.zeros((m, n), np.int64)
    present = np.zeros((m, w64(n)), np.uint64)
    scale = np.full(m, 3, np.int32)
    for j, name in enumerate(metric_names):
        items = [(index[node], q) for node, q in metrics.get(name, {}).items() if node in index]
        k = max([quantity_decimals(q) for _, q in items], default=0)
        scale[j] = max(k, 3)  # milli unless a value needs more places
        for i, q in items:
            try:
                v[j, i] = quantity_to_scaled(q, int(scale[j]))
            except _lib.PasError as e:
                if e.code != _lib.PAS_ENOTEXACT:
                    raise
                raise _lib.PasError(e.code, f"metric {name!r}: {q!r} at 10^-{scale[j]} is "
                                            "outside int64") from None
            present[j, i >> 6] |= np.uint64(1 << (i & 63))
    return v, present, scale


def tas_snapshot_from_metrics_wide(metrics: Mapping[str, Mapping[str, str]],
                                   node_names: Sequence[str],
                                   metric_names: Optional[Sequence[str]] = None):
    """(v, present, scale, wide) for Context.tas_snapshot_set_wide: every column on which
    tas_snapshot_from_metrics succeeds is exactly that function's column; any other column
    (its values do not all fit int64 at one decimal scale) is zero in v, keeps its presence
    bits, and has an entry wide[m] = (whole [N] int64, nano [N] uint32), value = whole +
    nano * 1e-9 with whole the floor (pas_quantity_to_wide).  PasError(PAS_ENOTEXACT), naming
    the metric, only for a value whose integer part is outside int64."""
    metric_names = list(metrics) if metric_names is None else list(metric_names)
    index = {n: i for i, n in enumerate(node_names)}
    n, m = len(node_names), len(metric_names)
    v = np.zeros((m, n), np.int64)
    present = np.zeros((m, w64(n)), np.uint64)
    scale = np.full(m, 3, np.int32)
    wide = {}
    for j, name in enumerate(metric_names):
        try:
            cv, cp, cs = tas_snapshot_from_metrics(metrics, node_names, [name])
            v[j], present[j], scale[j] = cv[0], cp[0], cs[0]
            continue
        except _lib.PasError as e:
            if e.code != _lib.PAS_ENOTEXACT:
                raise
        whole = np.zeros(n, np.int64)
        nano = np.zeros(n, np.uint32)
        for node, q in metrics.get(name, {}).items():
            if node not in index:
                continue
            i = index[node]
            try:
                whole[i], nano[i] = quantity_to_wide(q)
            except _lib.PasError as e:
                if e.code != _lib.PAS_ENOTEXACT:
                    raise
                raise _lib.PasError(e.code, f"metric {name!r}: the integer part of {q!r} is "
                                            "outside int64") from None
            present[j, i >> 6] |= np.uint64(1 << (i & 63))
        wide[j] = (whole, nano)
    return v, present, scale, wide


def pack_literals(metrics: Mapping[str, Mapping[str, str]], order: Sequence[str]):
    """(col_off int64 [len(order) + 1], nodes, lit_off int64 [T + 1], blob bytes): the maps of
    the metrics `order` names, one entry per (node, quantity) in the maps' own order, the
    literals end to end in one blob and the entries' node names in the list `nodes`.  Nothing
    is parsed."""
    col_off = np.zeros(len(order) + 1, np.int64)
    nodes: List[str] = []
    lits: List[bytes] = []
    for j, name in enumerate(order):
        mp = metrics.get(name) or {}
        nodes.extend(mp)
        lits.extend(q.encode() if isinstance(q, str) else bytes(q) for q in mp.values())
        col_off[j + 1] = len(nodes)
    lit_off = np.zeros(len(lits) + 1, np.int64)
    np.cumsum(np.fromiter(map(len, lits), np.int64, len(lits)), out=lit_off[1:])
    return col_off, nodes, lit_off, b"".join(lits)


def pack_quantities(metrics: Mapping[str, Mapping[str, str]], node_index: Mapping[str, int],
                    order: Sequence[str]):
    """(col_off, entry_node int32 [T], lit_off, blob) for Context.tas_snapshot_update_quantities:
    pack_literals with every entry's node name looked up in node_index (-1 for a name without a
    slot: its literal is still validated, and it takes no part in the column).  No parsing."""
    col_off, nodes, lit_off, blob = pack_literals(metrics, order)
    entry_node = np.fromiter((node_index.get(n, -1) for n in nodes), np.int32, len(nodes))
    return col_off, entry_node, lit_off, blob


def pack_names(nodes: Sequence):
    """(name_off int64 [len(nodes) + 1], blob bytes) of node names end to end, for the name
    table's calls (Context.names_set / names_resolve / names_assign /
    tas_snapshot_update_quantities_names).  ASCII names, where the string length is the byte
    length, take one join, one encode and one pass of len; anything else (non-ASCII str, bytes,
    None for a spare slot = the empty name) is encoded name by name."""
    n = len(nodes)
    off = np.zeros(n + 1, np.int64)
    try:
        joined = "".join(nodes)
        ascii_only = joined.isascii()
    except TypeError:
        ascii_only = False
    if ascii_only:
        blob = joined.encode()
        np.cumsum(np.fromiter(map(len, nodes), np.int64, n), out=off[1:])
        return off, blob
    enc = [b"" if s is None else s.encode() if isinstance(s, str) else bytes(s) for s in nodes]
    np.cumsum(np.fromiter(map(len, enc), np.int64, n), out=off[1:])
    return off, b"".join(enc)


def pack_card_names(card_names: Sequence[Sequence], parked: Optional[Sequence[Sequence]],
                    k: int):
    """(name_off int64 [len(card_names) * k + 1], blob bytes) for the card-name table's calls
    (Context.gas_card_names_set / gas_card_names_update): row s is card_names[s] followed by
    parked[s] (parked may be None), padded with empty names to k entries.  A row of more than k
    names is a ValueError."""
    flat: List = []
    for s, cards in enumerate(card_names):
        row = list(cards) + (list(parked[s]) if parked is not None else [])
        if len(row) > k:
            raise ValueError(f"row {s}: {len(row)} card names > k = {k}")
        flat.extend(row)
        flat.extend([""] * (k - len(row)))
    return pack_names(flat)


def pack_node_strings(nodes: Sequence[Optional[dict]], kinds: Sequence[str]):
    """(states int32 [U], label_off int64 [U + 1], label_blob, cap_off int64 [U * Q + 1],
    cap_blob) for Context.gas_nodes_update_strings[_names]: per node dict as gas_node_row reads
    it ({"labels": ..., "allocatable": ...}, or None for a node the lister does not know) its
    state (PAS_GAS_NODE_GONE / NO_LABEL / LABEL), its cards label as it is and one allocatable
    literal per kind (empty for a kind the node does not advertise or that is no
    "gpu.intel.com/" resource).  Nothing is split, sorted or parsed."""
    states = np.zeros(len(nodes), np.int32)
    labels: List = []
    lits: List = []
    for i, node in enumerate(nodes):
        node_labels = (node.get("labels") or {}) if node is not None else {}
        listed = node is not None and GPU_LIST_LABEL in node_labels
        states[i] = (_lib.PAS_GAS_NODE_GONE if node is None else
                     _lib.PAS_GAS_NODE_LABEL if listed else _lib.PAS_GAS_NODE_NO_LABEL)
        labels.append(node_labels[GPU_LIST_LABEL] if listed else "")
        alloc = (node.get("allocatable") or {}) if listed else {}
        lits.extend(alloc[k] if k in alloc and k.startswith(RESOURCE_PREFIX) else ""
                    for k in kinds)
    return (states,) + pack_names(labels) + pack_names(lits)


def go_sort_strings(names):
    """sort.Strings: bytewise order of the UTF-8 encodings ("card10" < "card2")."""
    return sorted(names, key=lambda s: s.encode())


def gas_snapshot_from_nodes(nodes: Sequence[Optional[dict]], kinds: Sequence[str],
                            max_cards: int = _lib.PAS_GAS_MAX_CARDS):
    """(n_cards [N] int32, cap_per_gpu [N][Q] int64, used [N][K][Q] int64, card_names) from
    per-node dicts {"labels": {...}, "allocatable": {resource: quantity}, "usage":
    {card: {resource: int}}}, or None for a node the lister does not know.  card_names[n]
    lists the node's cards in rank order (rank = the 3-bit index in a pas_gas_fit word, or the
    byte of a pas_gas_selection record).  K is the largest card count of the nodes (at least
    1); a node with more than max_cards cards is PAS_ECAPACITY."""
    q = len(kinds)
    n = len(nodes)
    n_cards = np.zeros(n, np.int32)
    cap = np.zeros((n, q), np.int64)
    card_names: List[List[str]] = []
    for i, node in enumerate(nodes):
        n_cards[i], cap[i], cards = gas_node_row(node, kinds)
        if len(cards) > max_cards:
            raise _lib.PasError(_lib.PAS_ECAPACITY,
                                f"node {i}: {len(cards)} cards > {max_cards} (PAS_GAS_MAX_CARDS)")
        card_names.append(cards)
    k = max([1] + [len(c) for c in card_names])
    used = np.zeros((n, k, q), np.int64)
    for i, node in enumerate(nodes):
        if n_cards[i] <= 0:
            continue
        usage: Dict[str, Dict[str, int]] = node.get("usage") or {}
        for r, card in enumerate(card_names[i]):
            for j, kind in enumerate(kinds):
                used[i, r, j] = int(usage.get(card, {}).get(kind, 0))
    return n_cards, cap, used, card_names


def gas_node_row(node: Optional[dict], kinds: Sequence[str]):
    """(n_cards, cap_per_gpu [Q] int64, cards) of one node dict as gas_snapshot_from_nodes reads
    it ({"labels": ..., "allocatable": ...}, or None for a node the lister does not know):
    its row of n_cards / cap_per_gpu and its label cards in rank order.  The card count is not
    checked against a snapshot's max_cards."""
    cap = np.zeros(len(kinds), np.int64)
    labels = (node.get("labels") or {}) if node is not None else {}
    if node is None or GPU_LIST_LABEL not in labels:
        return (-1 if node is None else 0), cap, []
    cards = go_sort_strings(set(labels[GPU_LIST_LABEL].split(".")))
    gpu_count = len(labels[GPU_LIST_LABEL].split("."))
    alloc = node.get("allocatable") or {}
    for j, kind in enumerate(kinds):
        if kind in alloc and kind.startswith(RESOURCE_PREFIX):
            # resourceMap.divide: Go integer division truncates toward zero
            value = quantity_as_int64(alloc[kind])
            share = abs(value) // gpu_count
            cap[j] = -share if value < 0 else share
    return len(cards), cap, cards


def card_remap(old_slots: Sequence[str], new_label_cards: Sequence[str], max_cards: int):
    """The slot map of a node whose label now lists new_label_cards, for
    pas_gas_nodes_update: (src [max_cards], new_slots, dropped).

    old_slots / new_slots name the cards of the row's slots: the label cards in sort.Strings
    order, then the parked cards (cards with usage the label does not list at the moment;
    the reference keeps them by name in nodeStatuses).  src[k] is the old slot whose usage
    slot k takes, -1 for a card first seen (zero usage) and for the unused slots.  Cards that
    leave the label are parked behind the label cards; parked cards the label lists again
    return to their rank with their usage.  The parked cards stay ordered most recently parked
    first; when label and parked cards exceed max_cards the oldest parked cards that do not
    fit are dropped and returned (their usage is lost, where the reference would remember it).
    Parking never needs more than max_cards slots; a label of more than max_cards cards is a
    ValueError (the snapshot has to grow first)."""
    label = go_sort_strings(set(new_label_cards))
    if len(label) > max_cards:
        raise ValueError(f"{len(label)} label cards > max_cards {max_cards}")
    listed = set(label)
    # cards that just left the label stand before the cards parked earlier
    parked = [c for c in old_slots if c not in listed]
    keep = max_cards - len(label)
    parked, dropped = parked[:keep], parked[keep:]
    new_slots = label + parked
    old_index = {c: k for k, c in enumerate(old_slots)}
    src = [old_index.get(c, -1) for c in new_slots] + [-1] * (max_cards - len(new_slots))
    return src, new_slots, dropped


def annotation(word: int, container_i915: Sequence[int], card_names: Sequence[str],
               selection=None) -> str:
    """The "gas-container-cards" annotation (scheduler.go:317-335) of a pas_gas_fit word:
    container c takes its next container_i915[c] selections; cards joined by ",", containers
    by "|".  A PAS_GAS_SEL_EXTENDED word needs its selection (the card ranks of its
    pas_gas_selection record, or of pas_gas_bind_ex)."""
    s_field = (int(word) >> 24) & 15
    if selection is not None:
        ranks = [int(r) for r in selection]
    elif s_field == _lib.PAS_GAS_SEL_EXTENDED:
        raise ValueError("PAS_GAS_SEL_EXTENDED word: pass its selection record")
    else:
        ranks = [(int(word) >> (3 * s)) & 7 for s in range(s_field)]
    out, pos = [], 0
    for n in container_i915:
        out.append(",".join(card_names[r] for r in ranks[pos:pos + n]))
        pos += n
    return "|".join(out)


def annotation_counts(counts, n_containers: int, card_names: Sequence[str]) -> str:
    """The "gas-container-cards" annotation from pas_gas_bind_counts' counts [C][K]: container
    c lists card k counts[c][k] times, in card order (its selections' order: first fit with
    one per-GPU request never returns to a card it has passed, scheduler.go:200-257)."""
    out = []
    for c in range(int(n_containers)):
        out.append(",".join(card_names[k] for k in range(len(card_names))
                            for _ in range(int(counts[c][k]))))
    return "|".join(out)


def parse_annotation(annotation: str, card_names: Sequence[str]):
    """The inverse of annotation(): (cards_per_container, ranks) of a "gas-container-cards"
    value as adjustPodResources reads it (node_resource_cache.go:241,253-256): strings.Split
    on "|" gives the containers' segments (one for "", as Go's Split does), strings.Split on
    "," a segment's card names.  An empty segment is 0 cards.  ranks lists the containers'
    cards consecutively as ranks into card_names (the node's label cards in rank order); a
    name not in card_names, the "" inside "a,,b" included, is rank -1 and still counts towards
    its container's numCards."""
    rank = {name: r for r, name in enumerate(card_names)}
    cards_per_container, ranks = [], []
    for segment in annotation.split("|"):
        names = segment.split(",") if segment else []
        cards_per_container.append(len(names))
        ranks.extend(rank.get(name, -1) for name in names)
    return cards_per_container, ranks
