"""TasCache: the reference cache's metric half over the device-resident TAS snapshot.

AutoUpdatingCache (telemetry-aware-scheduling/pkg/cache/autoupdating.go) keeps one node map
per metric name under "metrics/<name>" and a registration count per name in metricMap.  The
controller registers the metric of every rule of a new policy (controller.go:83-87,142-146 ->
WriteMetric(name, nil)) and unregisters it with the policy (:129-133,163-167 -> DeleteMetric);
the periodic refresh replaces the whole map of every registered name (:46-72).  Here the same
decisions are made on the host and the maps live on the device: a name with data owns a metric
column, a node name owns a node slot, and what changes the shape goes through
pas_tas_snapshot_reshape, so a new node or a new metric never re-uploads or re-sorts the
columns that did not change.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Mapping, Optional, Sequence, Set

import numpy as np

from . import _lib
from .context import quantity_to_wide, w64
from .snapshot import pack_literals, pack_names, tas_snapshot_from_metrics_wide

METRIC_GROWTH = 8  # columns added when no free column is left


class TasCache:
    """AutoUpdatingCache's metric half over a context's resident TAS snapshot, as GasCache is
    for the GAS cache.  Single-threaded: the reference serialises through its actor and mtx.

    `ctx` holds the snapshot of generation `gen` over `node_names` (slot -> name, None for a
    spare slot) x `metric_names` (column -> name, None for a free column) with the recorded
    column scales `scale` and the wide columns marked in `wide`.  Every device call moves gen
    by one.  metric_index holds a name only while the name has data: a registered name without
    data is "no metric found" in ReadMetric (autoupdating.go:76-85), so its rules must see
    metric -1, as MetricsExtender._rules gives for an unknown name
    (MetricsExtender.snapshot_changed takes gen, node_names and metric_names).

    The reference's quirks are restated as they are.
      write_metric(name, data=None)   WriteMetric (:105-116) with the actor's write
          (cache.go:51-58).  Empty or None data keeps whatever the name holds and adds one to
          its registration count (the first time: sets it to 1).  Non-empty data replaces the
          whole map and leaves the count alone, so a name written with data but never
          registered is never refreshed.
      delete_metric(name)             DeleteMetric (:127-137).  Count exactly 1: registration
          and data go and the column becomes free.  Otherwise the count drops by one, also
          for a name never registered (it becomes -1) and for counts <= 0; such a name stays
          registered, is still refreshed, and is only removed when its count is exactly 1
          again.
      update_all_metrics(fetch)       updateAllMetrics / updateMetric (:46-72).  fetch(name)
          returns {node: quantity string} or raises.  Every registered name, whatever its
          count: the empty name is unregistered (its data stays); a raise leaves the column
          as it is; anything else goes through write_metric(name, result), so an empty result
          keeps the data and bumps the count.

    The device side.  A node name first seen takes a spare slot; when none is left the
    snapshot grows by max(64, N / 8) slots rounded up to 64 (GasCache's rule).  A name with
    first data takes a free column; when none is left the snapshot grows by 8 columns.  A
    column freed by delete_metric is emptied (no present bit, milli, narrow) and reused.  A
    node that no metric lists any more keeps its slot until compact() drops it; nothing calls
    compact() implicitly.  One refresh issues at most one
    pas_tas_snapshot_reshape for all its new nodes and columns, then at most one
    pas_tas_snapshot_update for its narrow columns, one pas_tas_snapshot_update_wide for its
    wide ones, and one pas_tas_snapshot_set_scale when a narrow column's scale changed (a
    column update keeps the recorded scale; nothing evaluates between the calls).  Columns are
    encoded as snapshot.tas_snapshot_from_metrics_wide encodes them: the same scale choice,
    wide only where narrow does not fit.  A wide column keeps the scale recorded before it
    became wide (pas_tas_snapshot_set_scale ignores wide columns; no compare reads it).
    Quantities are checked before anything changes: a value whose integer part is outside
    int64 raises PasError(PAS_ENOTEXACT) and leaves cache and snapshot as they were.

    Combined TAS + GAS contexts need both snapshots to hold the same slots.  `slots` is any
    object with node_index and node_names (a GasCache is one), consulted read-only: with it
    the cache never picks a slot itself, follows slots.node_names at every flush (reshaping
    to len(slots.node_names) when that is larger), and leaves out metric entries of names
    that have no slot there, listing them in skipped_nodes.  Such a node fails the GAS fit
    anyway (FetchNode error); the TAS-only verbs treat it as a node unknown to the snapshot
    (it passes the filter and is left out of the prioritize list).  A skipped entry is
    installed by the first refresh of its metric after the name got a slot.

    device_ingest=True hands the Quantity strings to the device as they are
    (pas_tas_snapshot_update_quantities): no value is parsed on the host.  One write or refresh
    then issues one pas_quantities_to_wide over all its literals, before anything changes (a
    literal that cannot be held raises PasError naming the metric and the literal and leaves
    cache and snapshot as they were, as above), at most one reshape, and one
    pas_tas_snapshot_update_quantities for all its columns, in place of the narrow update, the
    wide update and the set_scale; `scale` and `wide` follow what that call reports.  The
    snapshot it installs is the same.

    device_names=True (with device_ingest=True and slots=None, ValueError otherwise) also leaves
    the node names to the device: the context's resident name table (pas_names_set, installed by
    from_metrics; a cache built by hand expects the table to hold node_names) owns the slot
    choice above.  After the literals are checked, one write or refresh issues one
    pas_names_assign over its entries' names (first-seen names take the spare slots; when they
    do not suffice the slot count grows by the rule above, pas_names_resize, and the assign is
    repeated), updates node_names / node_index for the new names only, then at most one reshape
    and one pas_tas_snapshot_update_quantities_names.  No dictionary is probed per entry.
    compact() also applies its map to the table (pas_names_remap).  An empty node name in a
    map raises ValueError before anything changes: the empty name marks a spare slot."""

    def __init__(self, ctx, gen: int, node_names: Sequence[Optional[str]],
                 metric_names: Sequence[Optional[str]], scale=None, wide=None, slots=None,
                 device_ingest: bool = False, device_names: bool = False):
        if device_names and (not device_ingest or slots is not None):
            raise ValueError("device_names needs device_ingest=True and slots=None")
        self.ctx, self.gen = ctx, gen
        self.slots = slots
        self.device_ingest = bool(device_ingest)
        self.device_names = bool(device_names)
        self._undo: Dict[str, tuple] = {}  # device_ingest: data a pending write replaced
        self.node_names: List[Optional[str]] = list(node_names)
        self.node_index: Dict[str, int] = {n: i for i, n in enumerate(node_names)
                                           if n is not None}
        self.metric_names: List[Optional[str]] = list(metric_names)
        self.metric_index: Dict[str, int] = {m: i for i, m in enumerate(metric_names)
                                             if m is not None}
        m = len(self.metric_names)
        self.scale: List[int] = [3] * m if scale is None else [int(s) for s in scale]
        self.wide: List[bool] = [False] * m if wide is None else [bool(x) for x in wide]
        self.counts: Dict[str, int] = {}  # metricMap
        self.data: Dict[str, Optional[Dict[str, str]]] = {}  # the "metrics/<name>" entries
        self.skipped_nodes: Set[str] = set()

    @classmethod
    def from_metrics(cls, ctx, gen: int, metrics: Mapping[str, Mapping[str, str]],
                     node_names: Optional[Sequence[str]] = None, spare_nodes: int = 0,
                     spare_metrics: int = 0, slots=None,
                     device_ingest: bool = False, device_names: bool = False) -> "TasCache":
        """A cache over a first snapshot, uploaded as generation gen: every entry of `metrics`
        as write_metric would take it (a non-empty map is data without a registration, an
        empty one a registration without data), over node_names (default: the maps' nodes in
        order of first appearance) plus spare_nodes spare slots and spare_metrics free
        columns.  device_names: the context's name table is installed over the same slots."""
        if device_names and (not device_ingest or slots is not None):
            raise ValueError("device_names needs device_ingest=True and slots=None")
        if slots is not None:
            names: List[Optional[str]] = list(slots.node_names)
        else:
            if node_names is None:
                node_names = list(dict.fromkeys(n for mp in metrics.values() for n in (mp or {})))
            names = list(node_names) + [None] * int(spare_nodes)
        if device_names and "" in names:
            raise ValueError("device_names: the empty node name marks a spare slot")
        held = [name for name, mp in metrics.items() if mp]
        v, p, scale, wide = tas_snapshot_from_metrics_wide(metrics, names, held)
        extra = int(spare_metrics)
        v = np.concatenate([v, np.zeros((extra, v.shape[1]), np.int64)])
        p = np.concatenate([p, np.zeros((extra, p.shape[1]), np.uint64)])
        scale = np.concatenate([scale, np.full(extra, 3, np.int32)])
        ctx.tas_snapshot_set_wide(gen, v, p, scale, wide)
        cols = held + [None] * extra
        if device_names:
            ctx.names_set(*pack_names(names))
        self = cls(ctx, gen, names, cols, scale, [c in wide for c in range(len(cols))], slots,
                   device_ingest, device_names)
        for name, mp in metrics.items():
            if mp:
                self.data[name] = dict(mp)
                self._note_skipped(mp)
            else:
                self._register(name)
        return self

    # ------------------------------------------------------------ the reference's calls
    def write_metric(self, name: str, data: Optional[Mapping[str, str]] = None):
        """WriteMetric: a registration (no data), or a new map for the name."""
        pending: Dict[str, Dict[str, str]] = {}
        self._write(name, data, pending)
        self._flush(pending)

    def delete_metric(self, name: str):
        """DeleteMetric."""
        if self.counts.get(name) != 1:
            self.counts[name] = self.counts.get(name, 0) - 1
            return
        del self.counts[name]
        self.data.pop(name, None)
        col = self.metric_index.pop(name, None)
        if col is None:
            return
        # the column emptied: narrow, no present bit, milli again
        n = len(self.node_names)
        self.ctx.tas_snapshot_update(self.gen, self.gen + 1, [col], np.zeros((1, n), np.int64),
                                     np.zeros((1, w64(n)), np.uint64))
        self.gen += 1
        self.metric_names[col] = None
        self.wide[col] = False
        if self.scale[col] != 3:
            self.scale[col] = 3
            self.ctx.tas_snapshot_set_scale(self.gen, self.scale)

    def update_all_metrics(self, fetch: Callable[[str], Mapping[str, str]]):
        """updateAllMetrics: one refresh of every registered name through fetch."""
        pending: Dict[str, Dict[str, str]] = {}
        for name in list(self.counts):
            if name == "":
                del self.counts[name]
                continue
            try:
                result = fetch(name)
            except Exception:  # GetNodeMetric's error: logged, the metric stays as it is
                continue
            self._write(name, result, pending)
        self._flush(pending)

    def compact(self, src_node: Optional[Sequence[int]] = None,
                spare_nodes: int = 0) -> List[int]:
        """Drop the dead node slots with one pas_tas_snapshot_compact call and return the map
        applied: new slot j holds old slot map[j], or nothing for -1.

        Without a map (a cache that owns its slots): a slot is dead when it is spare or no held
        map in `data` lists its name, as the reference's maps forget a node one refresh after
        it left (autoupdating.go:62-72); the live slots keep their order and spare_nodes spare
        slots follow them.  With a map (the combined case: src = gas.compact();
        tas.compact(src)) exactly that map is applied.  A cache that follows `slots` does not
        choose: without a map it raises ValueError.  A name that lost its slot and comes back
        takes a fresh slot (or, with `slots`, is a skipped node until the slot owner has it
        again).  A MetricsExtender over this cache takes the new slots through
        snapshot_changed, as after a reshape."""
        if src_node is None:
            if self.slots is not None:
                raise ValueError("compact: the slot owner decides (pass its map)")
            listed = {n for mp in self.data.values() if mp for n in mp}
            src = [i for i, n in enumerate(self.node_names) if n is not None and n in listed]
            src += [-1] * int(spare_nodes)
        else:
            # (a slot the owner added since this cache's last flush holds no metric yet)
            n_old = len(self.node_names)
            src = [int(s) if s < n_old else -1 for s in src_node]
        self.ctx.tas_snapshot_compact(self.gen, self.gen + 1, src)
        self.gen += 1
        if self.device_names:
            self.ctx.names_remap(src)
        self.node_names = [self.node_names[s] if s >= 0 else None for s in src]
        self.node_index = {n: i for i, n in enumerate(self.node_names) if n is not None}
        if self.slots is not None:
            for mp in self.data.values():
                self._note_skipped(mp or {})
        return src

    # ------------------------------------------------------------ host side
    def _register(self, name: str):
        self.counts[name] = self.counts.get(name, 0) + 1 if name in self.counts else 1
        self.data.setdefault(name, None)

    def _write(self, name: str, data, pending):
        if not data:  # nilPayloadCheck: the payload is nil, the cache keeps what it has
            self._register(name)
            return
        if self.device_ingest:  # checked on the device, by _flush, before anything else changes
            self._undo.setdefault(name, (name in self.data, self.data.get(name)))
        else:
            for q in data.values():  # nothing changes when a value cannot be held
                quantity_to_wide(q)
        self.data[name] = dict(data)
        pending[name] = self.data[name]

    def _note_skipped(self, mp):
        if self.slots is not None:
            self.skipped_nodes.update(n for n in mp if n not in self.slots.node_index)

    def _flush(self, pending: Dict[str, Dict[str, str]]):
        """The device calls of one write or refresh: reshape, narrow update, wide update,
        set_scale, each at most once (device_ingest: see _flush_literals; device_names: the
        node slots come from _assign_names, after the literals are checked)."""
        if self.device_names and any("" in mp for mp in pending.values()):
            self._restore_undo()
            raise ValueError("device_names: the empty node name marks a spare slot")
        packed = self._check_literals(pending) if self.device_ingest and pending else None
        n_old, m_old = len(self.node_names), len(self.metric_names)
        # node slots
        name_off = name_blob = None
        if self.device_names:
            if pending:
                name_off, name_blob = pack_names(packed[2])
                self._assign_names(packed[2], name_off, name_blob)
        elif self.slots is not None:
            names = list(self.slots.node_names)
            names += [None] * (n_old - len(names))
            self.node_names = names
            self.node_index = {n: i for i, n in enumerate(names) if n is not None}
            self.skipped_nodes -= set(self.node_index)
            for mp in pending.values():
                self._note_skipped(mp)
        else:
            new = list(dict.fromkeys(n for mp in pending.values() for n in mp
                                     if n not in self.node_index))
            spare = [i for i, n in enumerate(self.node_names) if n is None] if new else []
            n = n_old
            while len(spare) < len(new):
                grown = n + (max(64, n // 8) + 63) // 64 * 64
                spare.extend(range(n, grown))
                n = grown
            self.node_names.extend([None] * (n - n_old))
            for name, slot in zip(new, spare):
                self.node_names[slot] = name
                self.node_index[name] = slot
        # metric columns
        first = [name for name in pending if name not in self.metric_index]
        free = [c for c, name in enumerate(self.metric_names) if name is None] if first else []
        while len(free) < len(first):
            m = len(self.metric_names)
            free.extend(range(m, m + METRIC_GROWTH))
            self.metric_names.extend([None] * METRIC_GROWTH)
            self.scale.extend([3] * METRIC_GROWTH)
            self.wide.extend([False] * METRIC_GROWTH)
        for name, col in zip(first, free):
            self.metric_names[col] = name
            self.metric_index[name] = col
        n, m = len(self.node_names), len(self.metric_names)
        if n != n_old or m != m_old:
            self.ctx.tas_snapshot_reshape(self.gen, self.gen + 1, n, m)
            self.gen += 1
        if not pending:
            return
        if packed is not None:
            self._flush_literals(*packed, name_off, name_blob)
            return
        # the columns, encoded as a from-scratch build encodes them
        order = sorted(pending, key=self.metric_index.__getitem__)
        v, p, scale, wide = tas_snapshot_from_metrics_wide(pending, self.node_names, order)
        narrow = [j for j in range(len(order)) if j not in wide]
        if narrow:
            cols = [self.metric_index[order[j]] for j in narrow]
            self.ctx.tas_snapshot_update(self.gen, self.gen + 1, cols, v[narrow], p[narrow])
            self.gen += 1
        if wide:
            js = sorted(wide)
            cols = [self.metric_index[order[j]] for j in js]
            self.ctx.tas_snapshot_update_wide(self.gen, self.gen + 1, cols,
                                              np.stack([wide[j][0] for j in js]),
                                              np.stack([wide[j][1] for j in js]), p[js])
            self.gen += 1
        rescale = False
        for j, name in enumerate(order):
            col = self.metric_index[name]
            self.wide[col] = j in wide
            if j not in wide and self.scale[col] != int(scale[j]):
                self.scale[col] = int(scale[j])
                rescale = True
        if rescale:
            self.ctx.tas_snapshot_set_scale(self.gen, self.scale)

    # ------------------------------------------------------------ device_ingest
    def _literal_error(self, code: int, at: int, order, col_off, nodes, lit_off, blob):
        j = int(np.searchsorted(col_off, at, side="right")) - 1
        lit = blob[int(lit_off[at]):int(lit_off[at + 1])].decode(errors="replace")
        what = ("the integer part of {!r} is outside int64" if code == _lib.PAS_ENOTEXACT
                else "{!r} is no resource.Quantity").format(lit)
        return _lib.PasError(code, f"metric {order[j]!r}, node {nodes[at]!r}: {what}")

    def _check_literals(self, pending):
        """The pending maps packed (snapshot.pack_literals, in pending's own order) and every
        literal parsed once on the device.  A literal that cannot be held: the maps the pending
        writes replaced are put back, nothing else has changed yet, PasError."""
        order = list(pending)
        col_off, nodes, lit_off, blob = pack_literals(pending, order)
        status = self.ctx.quantities_to_wide(lit_off, blob)[3]
        bad = np.flatnonzero(status)
        if bad.size:
            self._restore_undo()
            at = int(bad[0])
            raise self._literal_error(int(status[at]), at, order, col_off, nodes, lit_off, blob)
        self._undo = {}
        return order, col_off, nodes, lit_off, blob

    def _restore_undo(self):
        """The maps the pending writes replaced, put back."""
        undo, self._undo = self._undo, {}
        for name, (had, old) in undo.items():
            if had:
                self.data[name] = old
            else:
                self.data.pop(name, None)

    def _assign_names(self, nodes, name_off, name_blob):
        """device_names: the slots of a flush's first-seen nodes, chosen by one pas_names_assign
        over the entries' names (the table grows first when its spare slots do not suffice);
        node_names / node_index follow for the new names only."""
        n = len(self.node_names)
        try:
            _, new_entry, new_slot = self.ctx.names_assign(name_off, name_blob, len(nodes),
                                                           want_slots=False)
        except _lib.PasError as e:
            if e.code != _lib.PAS_ECAPACITY:
                raise
            spare = n - len(self.node_index)
            while spare < e.n_new:
                grown = n + (max(64, n // 8) + 63) // 64 * 64
                spare += grown - n
                n = grown
            self.ctx.names_resize(n)
            _, new_entry, new_slot = self.ctx.names_assign(name_off, name_blob, len(nodes),
                                                           want_slots=False)
        self.node_names.extend([None] * (n - len(self.node_names)))
        for entry, slot in zip(new_entry.tolist(), new_slot.tolist()):
            self.node_names[slot] = nodes[entry]
            self.node_index[nodes[entry]] = slot

    def _flush_literals(self, order, col_off, nodes, lit_off, blob, name_off=None,
                        name_blob=None):
        """One pas_tas_snapshot_update_quantities for the pending columns (slots and columns
        are assigned, the snapshot has its new shape); device_names: its _names form over the
        packed node names, no lookup on the host."""
        cols = [self.metric_index[name] for name in order]
        try:
            if name_off is not None:
                kind, scale, _ = self.ctx.tas_snapshot_update_quantities_names(
                    self.gen, self.gen + 1, cols, col_off, name_off, name_blob, lit_off, blob)
            else:
                index = self.node_index
                entry_node = np.fromiter((index.get(n, -1) for n in nodes), np.int32, len(nodes))
                kind, scale = self.ctx.tas_snapshot_update_quantities(
                    self.gen, self.gen + 1, cols, col_off, entry_node, lit_off, blob)
        except _lib.PasError as e:  # (_check_literals has parsed them all: not expected)
            at = getattr(e, "bad_entry", -1)
            if at < 0:
                raise
            raise self._literal_error(e.code, at, order, col_off, nodes, lit_off, blob) from None
        self.gen += 1
        for col, k, s in zip(cols, kind, scale):
            self.wide[col] = bool(k)
            self.scale[col] = int(s)
