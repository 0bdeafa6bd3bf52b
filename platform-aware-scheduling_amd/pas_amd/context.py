"""Thin Python handle over a pas_ctx (include/pas.h).

Host entry points take/return numpy arrays; *_device entry points take objects with a
``data_ptr()`` (torch tensors on the GPU) and a HIP stream handle, so benchmarks can run
with every input already resident in HBM.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_double, c_int32, c_int64, c_uint64, c_void_p
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import PasError

# pas_rule {int32 metric; int32 op; int64 target}
RULE_DTYPE = np.dtype([("metric", "<i4"), ("op", "<i4"), ("target", "<i8")], align=True)
assert RULE_DTYPE.itemsize == 16


def w64(n: int) -> int:
    return (n + 63) // 64


def make_rules(metric, op, target) -> np.ndarray:
    metric = np.asarray(metric, dtype=np.int32)
    r = np.zeros(metric.shape[0], dtype=RULE_DTYPE)
    r["metric"] = metric
    r["op"] = np.asarray(op, dtype=np.int32)
    r["target"] = np.asarray(target, dtype=np.int64)
    return r


def _ptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "arrays passed to libpas must be C-contiguous"
    return a.ctypes.data_as(c_void_p)


def _dptr(t):
    if t is None:
        return None
    return c_void_p(t.data_ptr())


PAS_STREAM_NULL = 1  # include/pas.h: the HIP null stream (NULL names the context's stream)


def _stream(s):
    """A hip_stream argument: None = the context's current stream; a torch.cuda.Stream or a raw
    handle otherwise, torch's default (null) stream as PAS_STREAM_NULL."""
    if s is None:
        return None
    h = s if isinstance(s, int) else s.cuda_stream
    return c_void_p(h if h != 0 else PAS_STREAM_NULL)


def parse_operator(op: str) -> int:
    """core.EvaluateRule's operator lookup (operator.go:14-25) via the C-ABI."""
    return _lib.load().pas_parse_operator(op.encode())


def quantity_to_milli(q: str) -> int:
    """Exact value*1000 of a resource.Quantity string; PasError(PAS_ENOTEXACT) otherwise."""
    out = c_int64()
    rc = _lib.load().pas_quantity_to_milli(q.encode(), byref(out))
    if rc != _lib.PAS_OK:
        raise PasError(rc, f"quantity {q!r}")
    return out.value


def quantity_to_scaled(q: str, places: int) -> int:
    """Exact value * 10^places (0..9) of a resource.Quantity string; PasError(PAS_ENOTEXACT)
    when that is not an integer or is outside int64."""
    out = c_int64()
    rc = _lib.load().pas_quantity_to_scaled(q.encode(), places, byref(out))
    if rc != _lib.PAS_OK:
        raise PasError(rc, f"quantity {q!r} at 10^-{places}")
    return out.value


def quantity_to_wide(q: str) -> Tuple[int, int]:
    """(whole, nano) of a resource.Quantity string: value = whole + nano * 1e-9 exactly, whole
    the floor, 0 <= nano < 10^9; PasError(PAS_ENOTEXACT) only when the integer part is outside
    int64."""
    whole = c_int64()
    nano = ctypes.c_uint32()
    rc = _lib.load().pas_quantity_to_wide(q.encode(), byref(whole), byref(nano))
    if rc != _lib.PAS_OK:
        raise PasError(rc, f"quantity {q!r}")
    return whole.value, nano.value


def quantity_decimals(q: str) -> int:
    """The fewest decimal places (0..9) that hold the parsed quantity exactly."""
    out = ctypes.c_int32()
    rc = _lib.load().pas_quantity_decimals(q.encode(), byref(out))
    if rc != _lib.PAS_OK:
        raise PasError(rc, f"quantity {q!r}")
    return out.value


def quantity_parse_fixed(q) -> Tuple[int, int, int, int, int]:
    """(status, whole, nano, decimals, fit) of one literal (str or bytes, no terminator needed)
    from the fixed-width parser the device runs (pas_quantity_parse_fixed): whole / nano as
    quantity_to_wide, decimals as quantity_decimals, fit the largest places at which
    quantity_to_scaled succeeds or -1.  The status is returned, not raised."""
    b = q.encode() if isinstance(q, str) else bytes(q)
    whole = c_int64()
    nano = ctypes.c_uint32()
    dec = ctypes.c_int32()
    fit = ctypes.c_int32()
    rc = _lib.load().pas_quantity_parse_fixed(b, len(b), byref(whole), byref(nano), byref(dec),
                                              byref(fit))
    return rc, whole.value, nano.value, dec.value, fit.value


def quantity_as_int64_fixed(q) -> Tuple[int, int]:
    """(status, value) of one literal (str or bytes, no terminator needed) from the fixed-width
    parser the device runs (pas_quantity_as_int64_fixed): value is quantity_as_int64's answer, the
    status is quantity_parse_fixed's and is returned, not raised."""
    b = q.encode() if isinstance(q, str) else bytes(q)
    out = c_int64()
    rc = _lib.load().pas_quantity_as_int64_fixed(b, len(b), byref(out))
    return rc, out.value


def gas_label_parse(label, cap: Optional[int] = None):
    """(n_pieces, n_cards, spans) of one "gpu.intel.com/cards" label (str or bytes, no terminator
    needed) from the routine the device runs (pas_gas_label_parse, csrc/label_fixed.h): the
    pieces of the split on ".", the distinct ones counted up to PAS_GAS_MAX_CARDS + 1, and the
    (begin, length) spans of the first cap cards (default: all counted) in rank order."""
    b = label.encode() if isinstance(label, str) else bytes(label)
    n = _lib.PAS_GAS_MAX_CARDS + 1 if cap is None else int(cap)
    spans = np.full((max(n, 1), 2), -7, np.int64)
    pieces, cards = c_int64(), ctypes.c_int32()
    rc = _lib.load().pas_gas_label_parse(b, len(b), byref(pieces), byref(cards), _ptr(spans), n)
    if rc != _lib.PAS_OK:
        raise PasError(rc, "pas_gas_label_parse")
    return pieces.value, cards.value, [tuple(x) for x in spans[:min(n, cards.value)].tolist()]


def name_hash(name) -> int:
    """pas_name_hash of a node name (str or bytes): the name table's hash, whose low bits pick
    the home bucket and whose high 32 bits are the tag (csrc/name_hash.h)."""
    b = name.encode() if isinstance(name, str) else bytes(name)
    return _lib.load().pas_name_hash(b, len(b))


def gas_annotation_parse(annotation, max_containers: Optional[int] = None,
                         cap: Optional[int] = None):
    """(n_segments, cards_per_container, n_listed, spans) of one "gas-container-cards" value
    (str or bytes, no terminator needed) from the routine the device runs
    (pas_gas_annotation_parse, csrc/annotation_fixed.h): the full segment and name counts, the
    counts of the first max_containers segments (default: all) and the (begin, length) spans
    of the first cap names (default: all)."""
    b = annotation.encode() if isinstance(annotation, str) else bytes(annotation)
    c = b.count(b"|") + 1 if max_containers is None else int(max_containers)
    n = len(b) + 1 if cap is None else int(cap)
    cpc = np.full(max(c, 1), -7, np.int32)
    spans = np.full((max(n, 1), 2), -7, np.int64)
    segs, listed = c_int64(), c_int64()
    rc = _lib.load().pas_gas_annotation_parse(b, len(b), c, byref(segs), _ptr(cpc), byref(listed),
                                              _ptr(spans), n)
    if rc != _lib.PAS_OK:
        raise PasError(rc, "pas_gas_annotation_parse")
    return (segs.value, cpc[:min(c, segs.value)].tolist(), listed.value,
            [tuple(x) for x in spans[:min(n, listed.value)].tolist()])


def gas_annotation_render(counts, card_names, n_cards: Optional[int] = None,
                          cap: Optional[int] = None) -> Tuple[int, bytes]:
    """(status, bytes) of one "gas-container-cards" value from counts [C][K] over the K names
    card_names (str or bytes), of which the first n_cards (default: all) are label cards, from
    the routine the device runs (pas_gas_annotation_render, csrc/annotation_fixed.h).  The
    status (PAS_GAS_OK / PAS_GAS_ERR_INPUT / PAS_GAS_ERR_OVERFLOW) is returned, not raised; a cap
    below the rendered length raises PasError(PAS_ECAPACITY) with the length in err.n_bytes."""
    names = [n.encode() if isinstance(n, str) else bytes(n) for n in card_names]
    k = len(names)
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1, k) if k else \
        np.zeros((len(counts), 0), np.int64)
    off = np.zeros(k + 1, np.int64)
    np.cumsum([len(n) for n in names], out=off[1:])
    blob = Context._blob(b"".join(names))
    l = _lib.load()
    status, n_bytes = c_int32(), c_int64()

    def call(buf, room):
        return l.pas_gas_annotation_render(
            counts.shape[0], k, k if n_cards is None else int(n_cards),
            _ptr(counts) if counts.size else None, _ptr(off), _ptr(blob), byref(status),
            _ptr(buf), room, byref(n_bytes))
    rc = call(None, 0)  # the sizing call
    if rc == _lib.PAS_ECAPACITY and (cap is None or cap >= n_bytes.value):
        buf = np.zeros(n_bytes.value if cap is None else max(int(cap), 1), np.uint8)
        rc = call(buf, len(buf))
        raw = buf[:n_bytes.value].tobytes()
    else:
        raw = b""
    if rc != _lib.PAS_OK:
        err = PasError(rc, "pas_gas_annotation_render")
        err.n_bytes = n_bytes.value
        raise err
    return status.value, raw


def quantity_as_int64(q: str) -> int:
    """resource.Quantity.AsInt64 with `ok` ignored (gpuscheduler/utils.go:23)."""
    out = c_int64()
    rc = _lib.load().pas_quantity_as_int64(q.encode(), byref(out))
    if rc != _lib.PAS_OK:
        raise PasError(rc, f"quantity {q!r}")
    return out.value


def label_patch_json(names, add_mask: int, remove_mask: int) -> bytes:
    """JSON PATCH body of one node's label update (deschedule/enforce.go:74-86, 104-135)."""
    l = _lib.load()
    arr = (ctypes.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    n = c_int64()
    cap = 256
    while True:
        buf = ctypes.create_string_buffer(cap)
        rc = l.pas_label_patch_json(len(names), arr, add_mask, remove_mask, buf, cap, byref(n))
        if rc == _lib.PAS_OK:
            return buf.raw[:n.value]
        if rc != _lib.PAS_ECAPACITY:
            raise PasError(rc, "pas_label_patch_json")
        cap = n.value


def label_patch_json_batch(names, add, rem) -> list:
    """The PATCH bodies of a whole patch list (pas_label_patch_json_batch): body i is
    label_patch_json(names, add[i], rem[i]), all rendered in one host call."""
    l = _lib.load()
    add = np.ascontiguousarray(add, dtype=np.uint64).reshape(-1)
    rem = np.ascontiguousarray(rem, dtype=np.uint64).reshape(-1)
    assert add.shape == rem.shape, "one add and one remove mask per record"
    n = add.shape[0]
    arr = (ctypes.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    off = np.zeros(n + 1, np.int64)
    total = c_int64()
    cap = 64 * n + 64
    while True:
        buf = ctypes.create_string_buffer(max(cap, 1))
        rc = l.pas_label_patch_json_batch(len(names), arr, n, _ptr(add), _ptr(rem), buf, cap,
                                          _ptr(off), byref(total))
        if rc == _lib.PAS_OK:
            raw, o = buf.raw, off.tolist()
            return [raw[o[i]:o[i + 1]] for i in range(n)]
        if rc != _lib.PAS_ECAPACITY:
            raise PasError(rc, "pas_label_patch_json_batch")
        cap = total.value


class Context:
    """One pas_ctx bound to a HIP device."""

    def __init__(self, device: int = -1, lib=None):
        self._l = lib if lib is not None else _lib.load()
        h = c_void_p()
        cfg = _lib.PasConfig(device, 0)
        rc = self._l.pas_create(byref(cfg), byref(h))
        if rc != _lib.PAS_OK:
            raise PasError(rc, "pas_create failed (no usable HIP device?)")
        self._h = h
        self.n_nodes = 0
        self.n_metrics = 0
        self.gas_shape = (0, 0, 0)

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "_h", None):
            self._l.pas_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str):
        if rc != _lib.PAS_OK:
            msg = self._l.pas_last_error(self._h)
            raise PasError(rc, f"{what}: {msg.decode() if msg else ''}")

    def last_error(self) -> str:
        return self._l.pas_last_error(self._h).decode()

    def set_stream(self, stream):
        self._check(self._l.pas_set_stream(self._h, _stream(stream)), "pas_set_stream")

    def synchronize(self):
        self._check(self._l.pas_synchronize(self._h), "pas_synchronize")

    # ------------------------------------------------------------------ timing
    def set_timing(self, level):
        """0/False = off, 1 = whole paths (PAS_TIMING_SPAN), 2/True = every launch."""
        level = 2 if level is True else int(level)
        self._check(self._l.pas_set_timing(self._h, level), "pas_set_timing")

    def kernel_time(self, kernel_id: int) -> Tuple[float, int]:
        ms = c_double()
        n = c_int64()
        self._check(self._l.pas_kernel_time(self._h, kernel_id, byref(ms), byref(n)),
                    "pas_kernel_time")
        return ms.value, n.value

    def reset_timing(self):
        self._check(self._l.pas_reset_timing(self._h), "pas_reset_timing")

    # ------------------------------------------------------------------ TAS
    def tas_snapshot_set(self, gen: int, v_milli: np.ndarray, present: np.ndarray,
                         scale=None):
        """Columns of value * 1000, or of value * 10^scale[m] (pas_tas_snapshot_set_scale)."""
        v = np.ascontiguousarray(v_milli, dtype=np.int64)
        m, n = v.shape
        p = np.ascontiguousarray(present, dtype=np.uint64)
        assert p.shape == (m, w64(n)), (p.shape, (m, w64(n)))
        self._check(self._l.pas_tas_snapshot_set(self._h, gen, n, m, _ptr(v), _ptr(p)),
                    "pas_tas_snapshot_set")
        self.n_nodes, self.n_metrics = n, m
        if scale is not None:
            self.tas_snapshot_set_scale(gen, scale)

    def tas_snapshot_set_scale(self, gen: int, scale, stream=None):
        """Decimal scale per column (0..9): column m holds value * 10^scale[m]."""
        sc = np.ascontiguousarray(scale, dtype=np.int32)
        self._check(self._l.pas_tas_snapshot_set_scale(self._h, gen, len(sc),
                                                       _ptr(sc) if sc.size else None,
                                                       _stream(stream)),
                    "pas_tas_snapshot_set_scale")

    def tas_snapshot_set_device(self, gen: int, n_nodes: int, n_metrics: int, v_t, p_t,
                                stream=None):
        self._check(self._l.pas_tas_snapshot_set_device(self._h, gen, n_nodes, n_metrics,
                                                        _dptr(v_t), _dptr(p_t),
                                                        _stream(stream)),
                    "pas_tas_snapshot_set_device")
        self.n_nodes, self.n_metrics = n_nodes, n_metrics

    def tas_snapshot_update(self, gen_from: int, gen_to: int, cols, v_milli: np.ndarray,
                            present: np.ndarray):
        """Replace metric columns `cols` (AutoUpdatingCache.updateMetric) and re-sort them."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        v = np.ascontiguousarray(v_milli, dtype=np.int64).reshape(len(cols), self.n_nodes)
        p = np.ascontiguousarray(present, dtype=np.uint64).reshape(len(cols), w64(self.n_nodes))
        self._check(self._l.pas_tas_snapshot_update(
            self._h, gen_from, gen_to, len(cols), _ptr(cols) if cols.size else None,
            _ptr(v) if v.size else None, _ptr(p) if p.size else None), "pas_tas_snapshot_update")

    def tas_snapshot_update_device(self, gen_from: int, gen_to: int, cols, v_t, p_t,
                                   stream=None):
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        self._check(self._l.pas_tas_snapshot_update_device(
            self._h, gen_from, gen_to, len(cols), _ptr(cols) if cols.size else None, _dptr(v_t),
            _dptr(p_t), _stream(stream)), "pas_tas_snapshot_update_device")

    def tas_snapshot_update_wide(self, gen_from: int, gen_to: int, cols, whole: np.ndarray,
                                 nano: np.ndarray, present: np.ndarray):
        """Replace metric columns `cols` with wide columns: value = whole + nano * 1e-9
        (pas_tas_snapshot_update_wide; whole int64, nano uint32 < 10^9, [len(cols)][N])."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        w = np.ascontiguousarray(whole, dtype=np.int64).reshape(len(cols), self.n_nodes)
        f = np.ascontiguousarray(nano, dtype=np.uint32).reshape(len(cols), self.n_nodes)
        p = np.ascontiguousarray(present, dtype=np.uint64).reshape(len(cols), w64(self.n_nodes))
        self._check(self._l.pas_tas_snapshot_update_wide(
            self._h, gen_from, gen_to, len(cols), _ptr(cols) if cols.size else None,
            _ptr(w) if w.size else None, _ptr(f) if f.size else None,
            _ptr(p) if p.size else None), "pas_tas_snapshot_update_wide")

    def tas_snapshot_update_wide_device(self, gen_from: int, gen_to: int, cols, whole_t, nano_t,
                                        p_t, stream=None):
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        self._check(self._l.pas_tas_snapshot_update_wide_device(
            self._h, gen_from, gen_to, len(cols), _ptr(cols) if cols.size else None,
            _dptr(whole_t), _dptr(nano_t), _dptr(p_t), _stream(stream)),
            "pas_tas_snapshot_update_wide_device")

    # ---- Quantity literals parsed on the device (csrc/tas_ingest.hip)
    @staticmethod
    def _blob(blob) -> np.ndarray:
        b = np.frombuffer(bytes(blob), dtype=np.uint8)
        return b if b.size else np.zeros(1, np.uint8)

    def quantities_to_wide(self, lit_off, blob):
        """(whole, nano, decimals, status) [n] of the literals blob[lit_off[i]:lit_off[i + 1]]
        (pas_quantities_to_wide): per literal what quantity_parse_fixed gives, whole and nano 0
        where the status is not PAS_OK."""
        off = np.ascontiguousarray(lit_off, dtype=np.int64).reshape(-1)
        n = len(off) - 1
        whole = np.zeros(max(n, 1), np.int64)
        nano = np.zeros(max(n, 1), np.uint32)
        dec = np.zeros(max(n, 1), np.int32)
        status = np.zeros(max(n, 1), np.int32)
        self._check(self._l.pas_quantities_to_wide(
            self._h, n, _ptr(off), _ptr(self._blob(blob)), _ptr(whole), _ptr(nano), _ptr(dec),
            _ptr(status)), "pas_quantities_to_wide")
        return whole[:n], nano[:n], dec[:n], status[:n]

    def quantities_to_wide_device(self, n: int, n_bytes: int, lit_off_t, bytes_t, whole_t, nano_t,
                                  dec_t, status_t, stream=None):
        self._check(self._l.pas_quantities_to_wide_device(
            self._h, n, n_bytes, _dptr(lit_off_t), _dptr(bytes_t), _dptr(whole_t), _dptr(nano_t),
            _dptr(dec_t), _dptr(status_t), _stream(stream)), "pas_quantities_to_wide_device")

    def _update_quantities_result(self, rc: int, what: str, bad, kind, scale):
        if rc != _lib.PAS_OK:
            msg = self._l.pas_last_error(self._h)
            err = PasError(rc, f"{what}: {msg.decode() if msg else ''}")
            err.bad_entry = bad.value  # -1 unless a literal failed to parse
            raise err
        return kind, scale

    def tas_snapshot_update_quantities(self, gen_from: int, gen_to: int, cols, col_off,
                                       entry_node, lit_off, blob):
        """Replace metric columns `cols` from Quantity literals (snapshot.pack_quantities):
        column cols[c] takes the entries [col_off[c], col_off[c + 1]), entry i the literal
        blob[lit_off[i]:lit_off[i + 1]] for node slot entry_node[i].  Returns (kind [n_cols]
        0 narrow / 1 wide, scale [n_cols]) as the device chose them.  A literal that does not
        parse raises PasError with its index in .bad_entry and changes nothing."""
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        c_off = np.ascontiguousarray(col_off, dtype=np.int64).reshape(-1)
        node = np.ascontiguousarray(entry_node, dtype=np.int32).reshape(-1)
        l_off = np.ascontiguousarray(lit_off, dtype=np.int64).reshape(-1)
        assert len(c_off) == len(cols) + 1 and len(l_off) == len(node) + 1
        kind = np.zeros(max(len(cols), 1), np.int32)
        scale = np.zeros(max(len(cols), 1), np.int32)
        bad = c_int64(-1)
        rc = self._l.pas_tas_snapshot_update_quantities(
            self._h, gen_from, gen_to, len(cols), _ptr(cols) if cols.size else None, _ptr(c_off),
            _ptr(node) if node.size else None, _ptr(l_off), _ptr(self._blob(blob)), _ptr(kind),
            _ptr(scale), byref(bad))
        return self._update_quantities_result(rc, "pas_tas_snapshot_update_quantities", bad,
                                              kind[:len(cols)], scale[:len(cols)])

    def tas_snapshot_update_quantities_device(self, gen_from: int, gen_to: int, cols, col_off,
                                              n_bytes: int, entry_node_t, lit_off_t, bytes_t,
                                              stream=None):
        """The same with entry_node / lit_off / bytes on the device (cols and col_off stay host
        arrays).  Synchronous on the stream."""
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        c_off = np.ascontiguousarray(col_off, dtype=np.int64).reshape(-1)
        assert len(c_off) == len(cols) + 1
        kind = np.zeros(max(len(cols), 1), np.int32)
        scale = np.zeros(max(len(cols), 1), np.int32)
        bad = c_int64(-1)
        rc = self._l.pas_tas_snapshot_update_quantities_device(
            self._h, gen_from, gen_to, len(cols), _ptr(cols) if cols.size else None, _ptr(c_off),
            n_bytes, _dptr(entry_node_t), _dptr(lit_off_t), _dptr(bytes_t), _ptr(kind),
            _ptr(scale), byref(bad), _stream(stream))
        return self._update_quantities_result(rc, "pas_tas_snapshot_update_quantities_device",
                                              bad, kind[:len(cols)], scale[:len(cols)])

    # ---- the resident node-name table (csrc/name_table.hip)
    @staticmethod
    def _csr(name_off):
        off = np.ascontiguousarray(name_off, dtype=np.int64).reshape(-1)
        assert len(off) >= 1, "offsets hold n + 1 entries"
        return off, len(off) - 1

    def names_set(self, name_off, blob):
        """Install the name table (pas_names_set): slot s holds blob[name_off[s]:name_off[s + 1]],
        an empty span is a spare slot (snapshot.pack_names).  A name in two slots is
        PasError(PAS_EINVAL) and leaves the previous table valid."""
        off, n = self._csr(name_off)
        self._check(self._l.pas_names_set(self._h, n, _ptr(off), _ptr(self._blob(blob))),
                    "pas_names_set")

    def names_info(self):
        """(n_slots, n_named, n_bytes) of the name table."""
        n, k, b = c_int32(), c_int32(), c_int64()
        self._check(self._l.pas_names_info(self._h, byref(n), byref(k), byref(b)),
                    "pas_names_info")
        return n.value, k.value, b.value

    def names_get(self):
        """(name_off int64 [n_slots + 1], blob bytes): the names packed in slot order."""
        n, _, nb = self.names_info()
        off = np.zeros(n + 1, np.int64)
        buf = np.zeros(max(nb, 1), np.uint8)
        self._check(self._l.pas_names_get(self._h, _ptr(off), _ptr(buf), nb), "pas_names_get")
        return off, buf[:nb].tobytes()

    def names_drop(self):
        self._check(self._l.pas_names_drop(self._h), "pas_names_drop")

    def names_resolve(self, name_off, blob) -> np.ndarray:
        """slot int32 [n] of the names blob[name_off[i]:name_off[i + 1]], -1 for a name without
        a slot (pas_names_resolve)."""
        off, n = self._csr(name_off)
        slot = np.full(max(n, 1), -1, np.int32)
        self._check(self._l.pas_names_resolve(self._h, n, _ptr(off), _ptr(self._blob(blob)),
                                              _ptr(slot)), "pas_names_resolve")
        return slot[:n]

    def names_resolve_device(self, n: int, n_bytes: int, name_off_t, bytes_t, slot_t,
                             stream=None):
        self._check(self._l.pas_names_resolve_device(
            self._h, n, n_bytes, _dptr(name_off_t), _dptr(bytes_t), _dptr(slot_t),
            _stream(stream)), "pas_names_resolve_device")

    def _assign_result(self, rc: int, what: str, n_new, new_entry, new_slot):
        if rc != _lib.PAS_OK:
            msg = self._l.pas_last_error(self._h)
            err = PasError(rc, f"{what}: {msg.decode() if msg else ''}")
            err.n_new = n_new.value  # PAS_ECAPACITY: the distinct new names
            raise err
        return new_entry[:n_new.value], new_slot[:n_new.value]

    def names_assign(self, name_off, blob, new_cap: Optional[int] = None, want_slots=True):
        """Lookup plus first-seen assignment (pas_names_assign): (slot int32 [n] or None,
        new_entry, new_slot), the latter two listing the first appearance of each new name and
        the spare slot it took.  PasError(PAS_ECAPACITY) carries .n_new and changes nothing."""
        off, n = self._csr(name_off)
        cap = n if new_cap is None else int(new_cap)
        slot = np.full(max(n, 1), -1, np.int32) if want_slots else None
        new_entry = np.zeros(max(cap, 1), np.int32)
        new_slot = np.zeros(max(cap, 1), np.int32)
        n_new = c_int64(0)
        try:
            rc = self._l.pas_names_assign(self._h, n, _ptr(off), _ptr(self._blob(blob)),
                                          _ptr(slot), cap, _ptr(new_entry), _ptr(new_slot),
                                          byref(n_new))
            new = self._assign_result(rc, "pas_names_assign", n_new, new_entry, new_slot)
        except PasError as e:
            e.slots = slot[:n] if slot is not None else None  # the plain lookups
            raise
        return (slot[:n] if slot is not None else None,) + new

    def names_assign_device(self, n: int, n_bytes: int, name_off_t, bytes_t, slot_t,
                            new_cap: Optional[int] = None, stream=None):
        """The same with the names and the slots on the device: (new_entry, new_slot)."""
        cap = n if new_cap is None else int(new_cap)
        new_entry = np.zeros(max(cap, 1), np.int32)
        new_slot = np.zeros(max(cap, 1), np.int32)
        n_new = c_int64(0)
        rc = self._l.pas_names_assign_device(
            self._h, n, n_bytes, _dptr(name_off_t), _dptr(bytes_t), _dptr(slot_t), cap,
            _ptr(new_entry), _ptr(new_slot), byref(n_new), _stream(stream))
        return self._assign_result(rc, "pas_names_assign_device", n_new, new_entry, new_slot)

    def names_resize(self, n_slots: int, stream=None):
        self._check(self._l.pas_names_resize(self._h, n_slots, _stream(stream)),
                    "pas_names_resize")

    def names_remap(self, src_slot, stream=None):
        """Renumber the table's slots with a compact map (pas_names_remap): new slot j holds
        the name of old slot src_slot[j], or is spare for -1."""
        src = np.ascontiguousarray(src_slot, dtype=np.int32).reshape(-1)
        self._check(self._l.pas_names_remap(self._h, len(src), _ptr(src) if src.size else None,
                                            _stream(stream)), "pas_names_remap")

    def tas_snapshot_update_quantities_names(self, gen_from: int, gen_to: int, cols, col_off,
                                             name_off, name_blob, lit_off, blob):
        """tas_snapshot_update_quantities with each entry's node given by name
        (snapshot.pack_names of the entries' node names): returns (kind, scale, n_unknown),
        n_unknown the entries whose name has no slot."""
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        c_off = np.ascontiguousarray(col_off, dtype=np.int64).reshape(-1)
        n_off = np.ascontiguousarray(name_off, dtype=np.int64).reshape(-1)
        l_off = np.ascontiguousarray(lit_off, dtype=np.int64).reshape(-1)
        assert len(c_off) == len(cols) + 1 and len(l_off) == len(n_off)
        kind = np.zeros(max(len(cols), 1), np.int32)
        scale = np.zeros(max(len(cols), 1), np.int32)
        bad, unknown = c_int64(-1), c_int64(0)
        rc = self._l.pas_tas_snapshot_update_quantities_names(
            self._h, gen_from, gen_to, len(cols), _ptr(cols) if cols.size else None, _ptr(c_off),
            _ptr(n_off), _ptr(self._blob(name_blob)), _ptr(l_off), _ptr(self._blob(blob)),
            _ptr(kind), _ptr(scale), byref(bad), byref(unknown))
        return self._update_quantities_result(
            rc, "pas_tas_snapshot_update_quantities_names", bad, kind[:len(cols)],
            scale[:len(cols)]) + (unknown.value,)

    def tas_snapshot_update_quantities_names_device(self, gen_from: int, gen_to: int, cols,
                                                    col_off, n_name_bytes: int, name_off_t,
                                                    name_bytes_t, n_bytes: int, lit_off_t,
                                                    bytes_t, stream=None):
        """The same with the name and literal arrays on the device.  Synchronous on the stream."""
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        c_off = np.ascontiguousarray(col_off, dtype=np.int64).reshape(-1)
        assert len(c_off) == len(cols) + 1
        kind = np.zeros(max(len(cols), 1), np.int32)
        scale = np.zeros(max(len(cols), 1), np.int32)
        bad, unknown = c_int64(-1), c_int64(0)
        rc = self._l.pas_tas_snapshot_update_quantities_names_device(
            self._h, gen_from, gen_to, len(cols), _ptr(cols) if cols.size else None, _ptr(c_off),
            n_name_bytes, _dptr(name_off_t), _dptr(name_bytes_t), n_bytes, _dptr(lit_off_t),
            _dptr(bytes_t), _ptr(kind), _ptr(scale), byref(bad), byref(unknown), _stream(stream))
        return self._update_quantities_result(
            rc, "pas_tas_snapshot_update_quantities_names_device", bad, kind[:len(cols)],
            scale[:len(cols)]) + (unknown.value,)

    def tas_snapshot_wide_count(self) -> int:
        """Number of wide columns of the resident snapshot."""
        n = c_int32()
        self._check(self._l.pas_tas_snapshot_wide_count(self._h, byref(n)),
                    "pas_tas_snapshot_wide_count")
        return n.value

    def tas_snapshot_set_wide(self, gen: int, v: np.ndarray, present: np.ndarray, scale, wide):
        """Install what snapshot.tas_snapshot_from_metrics_wide returns: the narrow columns at
        their scales, then the wide columns {m: (whole [N], nano [N])}, ending at generation
        gen.  The set itself carries an intermediate generation (gen with the top bit flipped)
        that no caller evaluates against; if the wide update fails the context is left without
        a TAS snapshot."""
        if not wide:
            self.tas_snapshot_set(gen, v, present, scale)
            return
        mid = gen ^ (1 << 63)
        cols = sorted(wide)
        whole = np.stack([np.asarray(wide[m][0], dtype=np.int64) for m in cols])
        nano = np.stack([np.asarray(wide[m][1], dtype=np.uint32) for m in cols])
        p = np.ascontiguousarray(present, dtype=np.uint64)
        self.tas_snapshot_set(mid, v, p, scale)
        try:
            self.tas_snapshot_update_wide(mid, gen, cols, whole, nano, p[cols])
        except Exception:
            self._l.pas_tas_snapshot_drop(self._h)
            raise

    def tas_snapshot_reshape(self, gen_from: int, gen_to: int, n_nodes: int, n_metrics: int,
                             src_col=None, stream=None):
        """Grow the node count and add, drop or move metric columns of the resident snapshot on
        the device (pas_tas_snapshot_reshape): new column m is old column src_col[m], or empty
        for -1; None keeps the old columns in place and appends empty ones."""
        src = None
        if src_col is not None:
            src = np.ascontiguousarray(src_col, dtype=np.int32)
            assert src.shape == (n_metrics,), (src.shape, n_metrics)
            if not src.size:  # an empty map (every column dropped) is still a map, not NULL
                src = np.zeros(1, np.int32)
        self._check(self._l.pas_tas_snapshot_reshape(
            self._h, gen_from, gen_to, n_nodes, n_metrics, _ptr(src), _stream(stream)),
            "pas_tas_snapshot_reshape")
        self.n_nodes, self.n_metrics = n_nodes, n_metrics

    def tas_snapshot_compact(self, gen_from: int, gen_to: int, src_node, stream=None):
        """Renumber the node slots of the resident snapshot on the device
        (pas_tas_snapshot_compact): new slot j holds old slot src_node[j], or nothing for -1; the
        old slots that src_node does not name are dropped.  The entries >= 0 are strictly
        increasing."""
        src = np.ascontiguousarray(src_node, dtype=np.int32).reshape(-1)
        self._check(self._l.pas_tas_snapshot_compact(
            self._h, gen_from, gen_to, len(src), _ptr(src) if src.size else None,
            _stream(stream)), "pas_tas_snapshot_compact")
        self.n_nodes = len(src)

    def tas_snapshot_get(self):
        """(gen, vals [M][N] int64, present [M][W64] uint64, scale [M] int32, wide [M] uint8,
        nano [M][N] uint32) of the resident snapshot (pas_tas_snapshot_get): present without
        bits past n_nodes, values and nanos meaningful only where the bit is set."""
        _, n, m = self.tas_snapshot_info()
        g = c_uint64()
        vals = np.zeros((m, n), np.int64)
        present = np.zeros((m, w64(n)), np.uint64)
        scale = np.zeros(m, np.int32)
        wide = np.zeros(m, np.uint8)
        nano = np.zeros((m, n), np.uint32)
        self._check(self._l.pas_tas_snapshot_get(self._h, byref(g), _ptr(vals), _ptr(present),
                                                 _ptr(scale), _ptr(wide), _ptr(nano)),
                    "pas_tas_snapshot_get")
        return g.value, vals, present, scale, wide, nano

    def tas_snapshot_info(self):
        g = c_uint64()
        n = c_int32()
        m = c_int32()
        self._check(self._l.pas_tas_snapshot_info(self._h, byref(g), byref(n), byref(m)),
                    "pas_tas_snapshot_info")
        return g.value, n.value, m.value

    def tas_eval(self, gen: int, rules: np.ndarray, rule_off: np.ndarray, prio: np.ndarray,
                 cand: Optional[np.ndarray] = None,
                 flags: int = _lib.PAS_TAS_FILTER | _lib.PAS_TAS_PRIORITIZE):
        """Returns (pass[P, W64] uint64 or None, order[P, N] int32 or None, len[P] or None)."""
        rule_off = np.ascontiguousarray(rule_off, dtype=np.int32)
        n_pods = rule_off.shape[0] - 1
        rules = np.ascontiguousarray(rules, dtype=RULE_DTYPE)
        prio = np.ascontiguousarray(prio, dtype=RULE_DTYPE)
        assert prio.shape[0] == n_pods
        n = self.n_nodes
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
            assert cand.shape == (n_pods, w64(n))
        pass_out = np.zeros((n_pods, w64(n)), np.uint64) if flags & _lib.PAS_TAS_FILTER else None
        order = np.zeros((n_pods, n), np.int32) if flags & _lib.PAS_TAS_PRIORITIZE else None
        lens = np.zeros(n_pods, np.int32) if flags & _lib.PAS_TAS_PRIORITIZE else None
        rc = self._l.pas_tas_eval(self._h, gen, n_pods, _ptr(rules) if rules.size else None,
                                  _ptr(rule_off), _ptr(prio), _ptr(cand), flags, _ptr(pass_out),
                                  _ptr(order), _ptr(lens))
        self._check(rc, "pas_tas_eval")
        return pass_out, order, lens

    def tas_eval_device(self, gen: int, n_pods: int, n_rules: int, rules_t, rule_off_t, prio_t,
                        cand_t, flags: int, pass_t, order_t, len_t, stream=None):
        rc = self._l.pas_tas_eval_device(self._h, gen, n_pods, n_rules, _dptr(rules_t),
                                         _dptr(rule_off_t), _dptr(prio_t), _dptr(cand_t), flags,
                                         _dptr(pass_t), _dptr(order_t), _dptr(len_t),
                                         _stream(stream))
        self._check(rc, "pas_tas_eval_device")

    def tas_prioritize_request(self, gen: int, prio, req_node) -> np.ndarray:
        """Request positions best-first for one extender request (pas_tas_prioritize_request,
        SURVEY.md A.3 tie order); req_node[j] = snapshot node of Items[j] or -1."""
        rule = np.ascontiguousarray(np.asarray(prio, dtype=RULE_DTYPE).reshape(1))
        req = np.ascontiguousarray(req_node, dtype=np.int32)
        pos = np.zeros(max(len(req), 1), np.int32)
        n = ctypes.c_int32(0)
        rc = self._l.pas_tas_prioritize_request(self._h, gen, _ptr(rule), len(req), _ptr(req),
                                                _ptr(pos), ctypes.byref(n))
        self._check(rc, "pas_tas_prioritize_request")
        return pos[: n.value]

    def tas_prioritize_request_device(self, gen: int, prio, n_req: int, req_t, pos_t, len_t,
                                      stream=None):
        rule = np.ascontiguousarray(np.asarray(prio, dtype=RULE_DTYPE).reshape(1))
        rc = self._l.pas_tas_prioritize_request_device(self._h, gen, _ptr(rule), n_req,
                                                       _dptr(req_t), _dptr(pos_t), _dptr(len_t),
                                                       _stream(stream))
        self._check(rc, "pas_tas_prioritize_request_device")

    # -- batches of requests in request terms (pas_tas_prioritize_requests and its kin):
    # req_off [R + 1] is the CSR of the requests' node lists, req_node their snapshot ids
    @staticmethod
    def _requests(req_off, req_node):
        req_off = np.ascontiguousarray(req_off, dtype=np.int32)
        req_node = np.ascontiguousarray(req_node, dtype=np.int32)
        lens = np.diff(req_off)
        return req_off, req_node, len(req_off) - 1, int(lens.max(initial=0))

    def tas_prioritize_requests(self, gen: int, req_off, prio, req_node):
        """(pos [T] int32, len [R] int32): request r's positions best-first at
        pos[req_off[r] : req_off[r] + len[r]], -1 after, each exactly
        tas_prioritize_request's list for that request."""
        req_off = np.ascontiguousarray(req_off, dtype=np.int32)
        req_node = np.ascontiguousarray(req_node, dtype=np.int32)
        prio = np.ascontiguousarray(prio, dtype=RULE_DTYPE)
        r = len(req_off) - 1
        assert prio.shape == (r,)
        pos = np.empty(max(len(req_node), 1), np.int32)  # (the call writes every position)
        lens = np.empty(max(r, 1), np.int32)
        rc = self._l.pas_tas_prioritize_requests(self._h, gen, r, _ptr(req_off), _ptr(prio),
                                                 _ptr(req_node), _ptr(pos), _ptr(lens))
        self._check(rc, "pas_tas_prioritize_requests")
        return pos[: len(req_node)], lens[:r]

    def tas_prioritize_requests_device(self, gen: int, req_off, prio, req_t, pos_t, len_t,
                                       stream=None):
        req_off = np.ascontiguousarray(req_off, dtype=np.int32)
        prio = np.ascontiguousarray(prio, dtype=RULE_DTYPE)
        rc = self._l.pas_tas_prioritize_requests_device(
            self._h, gen, len(req_off) - 1, _ptr(req_off), _ptr(prio), _dptr(req_t),
            _dptr(pos_t), _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_prioritize_requests_device")

    def tas_filter_requests(self, gen: int, req_off, rules, rule_off, req_node,
                            out: Optional[np.ndarray] = None) -> np.ndarray:
        """pass [R][ld] uint64: bit j of row r = request r's node at position j is unknown to
        the snapshot or violates none of rules[rule_off[r] : rule_off[r + 1]].  out: rows to
        write into (pitch out.shape[1]); words past a request's own are left as they are."""
        req_off, req_node, r, longest = self._requests(req_off, req_node)
        rules = np.ascontiguousarray(rules, dtype=RULE_DTYPE)
        rule_off = np.ascontiguousarray(rule_off, dtype=np.int32)
        assert rule_off.shape == (r + 1,)
        if out is None:
            out = np.zeros((r, max(w64(longest), 1)), np.uint64)
        assert out.dtype == np.uint64 and out.ndim == 2 and out.shape[0] == r
        rc = self._l.pas_tas_filter_requests(self._h, gen, r, _ptr(req_off),
                                             _ptr(rules) if rules.size else None,
                                             _ptr(rule_off), _ptr(req_node), _ptr(out),
                                             out.shape[1])
        self._check(rc, "pas_tas_filter_requests")
        return out

    def tas_filter_requests_device(self, gen: int, req_off, n_rules: int, rules_t, rule_off_t,
                                   req_t, pass_t, ld_words: int, stream=None):
        req_off = np.ascontiguousarray(req_off, dtype=np.int32)
        rc = self._l.pas_tas_filter_requests_device(
            self._h, gen, len(req_off) - 1, _ptr(req_off), n_rules, _dptr(rules_t),
            _dptr(rule_off_t), _dptr(req_t), _dptr(pass_t), ld_words, _stream(stream))
        self._check(rc, "pas_tas_filter_requests_device")

    def gas_fit_requests(self, gen: int, req_off, req_node, req: np.ndarray,
                         req_mask: np.ndarray, n_containers: np.ndarray, i915_index: int,
                         out: Optional[np.ndarray] = None) -> np.ndarray:
        """fit [R][ld] uint64: bit j of row r = pod r fits request r's node at position j (bit
        31 of the gas_fit word; 0 for a node the snapshot does not hold).  out as in
        tas_filter_requests."""
        req_off, req_node, r, longest = self._requests(req_off, req_node)
        req = np.ascontiguousarray(req, dtype=np.int64)
        p, c, q = req.shape
        req_mask = np.ascontiguousarray(req_mask, dtype=np.uint32)
        n_containers = np.ascontiguousarray(n_containers, dtype=np.int32)
        assert p == r and req_mask.shape == (p, c) and n_containers.shape == (p,)
        if out is None:
            out = np.zeros((r, max(w64(longest), 1)), np.uint64)
        assert out.dtype == np.uint64 and out.ndim == 2 and out.shape[0] == r
        rc = self._l.pas_gas_fit_requests(self._h, gen, r, _ptr(req_off), _ptr(req_node), c,
                                          i915_index, _ptr(req), _ptr(req_mask),
                                          _ptr(n_containers), _ptr(out), out.shape[1])
        self._check(rc, "pas_gas_fit_requests")
        return out

    def gas_fit_requests_device(self, gen: int, req_off, req_node_t, max_containers: int,
                                i915_index: int, req_t, mask_t, ncont_t, fit_t, ld_words: int,
                                stream=None):
        req_off = np.ascontiguousarray(req_off, dtype=np.int32)
        rc = self._l.pas_gas_fit_requests_device(
            self._h, gen, len(req_off) - 1, _ptr(req_off), _dptr(req_node_t), max_containers,
            i915_index, _dptr(req_t), _dptr(mask_t), _dptr(ncont_t), _dptr(fit_t), ld_words,
            _stream(stream))
        self._check(rc, "pas_gas_fit_requests_device")

    def tas_violations(self, gen: int, rules: np.ndarray, rule_off: np.ndarray) -> np.ndarray:
        rule_off = np.ascontiguousarray(rule_off, dtype=np.int32)
        s = rule_off.shape[0] - 1
        rules = np.ascontiguousarray(rules, dtype=RULE_DTYPE)
        out = np.zeros((s, w64(self.n_nodes)), np.uint64)
        rc = self._l.pas_tas_violations(self._h, gen, s, _ptr(rules) if rules.size else None,
                                        _ptr(rule_off), _ptr(out))
        self._check(rc, "pas_tas_violations")
        return out

    def tas_violations_device(self, gen: int, n_strat: int, n_rules: int, rules_t, rule_off_t,
                              viol_t, stream=None):
        rc = self._l.pas_tas_violations_device(self._h, gen, n_strat, n_rules, _dptr(rules_t),
                                               _dptr(rule_off_t), _dptr(viol_t),
                                               _stream(stream))
        self._check(rc, "pas_tas_violations_device")

    # -- the resident policy table (pas_tas_policies_set) and the verbs by policy id
    def tas_policies_set(self, rules, rule_off, prio):
        """Install the policy table: policy i owns rules[rule_off[i] : rule_off[i + 1]] as its
        dontschedule rules and prio[i] as its scheduleonmetric rule (metric < 0: none)."""
        rule_off = np.ascontiguousarray(rule_off, dtype=np.int32)
        n = len(rule_off) - 1
        rules = np.ascontiguousarray(rules, dtype=RULE_DTYPE)
        prio = np.ascontiguousarray(prio, dtype=RULE_DTYPE)
        assert prio.shape == (n,)
        rc = self._l.pas_tas_policies_set(self._h, n, _ptr(rules) if rules.size else None,
                                          _ptr(rule_off), _ptr(prio) if prio.size else None)
        self._check(rc, "pas_tas_policies_set")

    def tas_policies_info(self) -> Tuple[int, int]:
        """(n_policies, n_rules) of the resident table."""
        n, r = c_int32(), c_int32()
        rc = self._l.pas_tas_policies_info(self._h, byref(n), byref(r))
        if rc != _lib.PAS_OK:
            raise PasError(rc, "pas_tas_policies_info: no policy table")
        return n.value, r.value

    def tas_policies_drop(self):
        self._check(self._l.pas_tas_policies_drop(self._h), "pas_tas_policies_drop")

    def tas_policies_violated(self, gen: int) -> np.ndarray:
        """viol [n_policies][W64]: the cached violating sets of the table's policies."""
        n, _ = self.tas_policies_info()
        out = np.zeros((n, w64(self.n_nodes)), np.uint64)
        rc = self._l.pas_tas_policies_violated(self._h, gen, _ptr(out) if out.size else None)
        self._check(rc, "pas_tas_policies_violated")
        return out

    def tas_policies_violated_device(self, gen: int, viol_t, stream=None):
        rc = self._l.pas_tas_policies_violated_device(self._h, gen, _dptr(viol_t),
                                                      _stream(stream))
        self._check(rc, "pas_tas_policies_violated_device")

    def tas_eval_policies(self, gen: int, pod_policy, cand: Optional[np.ndarray] = None,
                          flags: int = _lib.PAS_TAS_FILTER | _lib.PAS_TAS_PRIORITIZE):
        """tas_eval with pod p's rules and prio taken from table row pod_policy[p] (-1: none).
        Returns (pass, order, len) as tas_eval."""
        pol = np.ascontiguousarray(pod_policy, dtype=np.int32).reshape(-1)
        n_pods, n = len(pol), self.n_nodes
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
            assert cand.shape == (n_pods, w64(n))
        pass_out = np.zeros((n_pods, w64(n)), np.uint64) if flags & _lib.PAS_TAS_FILTER else None
        order = np.zeros((n_pods, n), np.int32) if flags & _lib.PAS_TAS_PRIORITIZE else None
        lens = np.zeros(n_pods, np.int32) if flags & _lib.PAS_TAS_PRIORITIZE else None
        rc = self._l.pas_tas_eval_policies(self._h, gen, n_pods, _ptr(pol), _ptr(cand), flags,
                                           _ptr(pass_out), _ptr(order), _ptr(lens))
        self._check(rc, "pas_tas_eval_policies")
        return pass_out, order, lens

    def tas_eval_policies_device(self, gen: int, n_pods: int, pod_policy_t, cand_t, flags: int,
                                 pass_t, order_t, len_t, stream=None):
        rc = self._l.pas_tas_eval_policies_device(self._h, gen, n_pods, _dptr(pod_policy_t),
                                                  _dptr(cand_t), flags, _dptr(pass_t),
                                                  _dptr(order_t), _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_eval_policies_device")

    def tas_filter_requests_policies(self, gen: int, req_off, req_policy, req_node,
                                     out: Optional[np.ndarray] = None) -> np.ndarray:
        """tas_filter_requests with request r's rules being table row req_policy[r]."""
        req_off, req_node, r, longest = self._requests(req_off, req_node)
        pol = np.ascontiguousarray(req_policy, dtype=np.int32)
        assert pol.shape == (r,)
        if out is None:
            out = np.zeros((r, max(w64(longest), 1)), np.uint64)
        assert out.dtype == np.uint64 and out.ndim == 2 and out.shape[0] == r
        rc = self._l.pas_tas_filter_requests_policies(self._h, gen, r, _ptr(req_off), _ptr(pol),
                                                      _ptr(req_node), _ptr(out), out.shape[1])
        self._check(rc, "pas_tas_filter_requests_policies")
        return out

    def tas_filter_requests_policies_device(self, gen: int, req_off, req_policy, req_t, pass_t,
                                            ld_words: int, stream=None):
        req_off = np.ascontiguousarray(req_off, dtype=np.int32)
        pol = np.ascontiguousarray(req_policy, dtype=np.int32)
        rc = self._l.pas_tas_filter_requests_policies_device(
            self._h, gen, len(req_off) - 1, _ptr(req_off), _ptr(pol), _dptr(req_t),
            _dptr(pass_t), ld_words, _stream(stream))
        self._check(rc, "pas_tas_filter_requests_policies_device")

    @staticmethod
    def _name_ids(names, n_strat: int):
        """int32 name ids of policy names (None: all distinct) as pas_tas_label_plan takes
        them: equal names, equal ids."""
        if names is None:
            return None
        assert len(names) == n_strat, "one policy name per strategy"
        ids = {}
        return np.array([ids.setdefault(n, len(ids)) for n in names], np.int32)

    def tas_label_plan(self, n_nodes: int, viol: np.ndarray, labels: Optional[np.ndarray] = None,
                       names=None):
        """(add [n_nodes] u64, remove [n_nodes] u64, total) of updateNodeLabels
        (deschedule/enforce.go:99-151) from viol[S][W64] and labels[S][W64] (or None);
        names[s] = policy name of strategy s (None: all distinct)."""
        viol = np.ascontiguousarray(viol, dtype=np.uint64)
        s = viol.shape[0]
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.uint64)
            assert labels.shape == viol.shape, "labels must have the shape of viol"
        ids = self._name_ids(names, s)
        add = np.zeros(n_nodes, np.uint64)
        rem = np.zeros(n_nodes, np.uint64)
        total = c_int64()
        rc = self._l.pas_tas_label_plan(self._h, n_nodes, s, _ptr(viol) if viol.size else None,
                                        _ptr(ids), _ptr(labels) if labels is not None and
                                        labels.size else None, _ptr(add), _ptr(rem),
                                        byref(total))
        self._check(rc, "pas_tas_label_plan")
        return add, rem, total.value

    def tas_label_plan_device(self, n_nodes: int, n_strat: int, viol_t, labels_t, add_t, rem_t,
                              total_t, stream=None, names=None):
        ids = self._name_ids(names, n_strat)
        rc = self._l.pas_tas_label_plan_device(self._h, n_nodes, n_strat, _dptr(viol_t),
                                               _ptr(ids), _dptr(labels_t), _dptr(add_t),
                                               _dptr(rem_t), _dptr(total_t), _stream(stream))
        self._check(rc, "pas_tas_label_plan_device")

    def tas_deschedule_device(self, gen: int, n_strat: int, n_rules: int, rules_t, rule_off_t,
                              viol_t, labels_t, add_t, rem_t, total_t, stream=None, names=None):
        """The sweep and its label plan in one pass (pas_tas_deschedule_device): viol_t as
        tas_violations_device, add_t / rem_t / total_t as tas_label_plan_device on it."""
        ids = self._name_ids(names, n_strat)
        rc = self._l.pas_tas_deschedule_device(self._h, gen, n_strat, n_rules, _dptr(rules_t),
                                               _dptr(rule_off_t), _dptr(viol_t), _ptr(ids),
                                               _dptr(labels_t), _dptr(add_t), _dptr(rem_t),
                                               _dptr(total_t), _stream(stream))
        self._check(rc, "pas_tas_deschedule_device")

    # -- the label plan as a patch list (pas_tas_label_patches, pas_tas_deschedule_patches)
    @staticmethod
    def _bitmaps(shape, **maps):
        """Optional [S][W64] bitmaps as contiguous uint64 arrays of `shape` (None stays None)."""
        out = []
        for what, m in maps.items():
            if m is not None:
                m = np.ascontiguousarray(m, dtype=np.uint64)
                assert m.shape == shape, f"{what} must have the shape of viol"
            out.append(m)
        return out

    @staticmethod
    def _patch_records(cap: int, out):
        """The record arrays of a host patch-list call: `out` = (node, add, rem) arrays of at
        least cap entries to write into (entries past the list stay as they are), else new."""
        if out is None:
            return np.zeros(cap, np.int32), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        node, add, rem = out
        assert node.dtype == np.int32 and add.dtype == np.uint64 and rem.dtype == np.uint64
        assert min(node.size, add.size, rem.size) >= cap, "record arrays shorter than cap"
        return node, add, rem

    def tas_label_patches(self, n_nodes: int, viol: np.ndarray,
                          labels: Optional[np.ndarray] = None, names=None,
                          violating: Optional[np.ndarray] = None,
                          null: Optional[np.ndarray] = None, cap: Optional[int] = None, out=None):
        """(node, add, rem, n_patches, total): the nodes whose patch body is not "[]" in
        ascending index with their masks (pas_tas_label_patches), from viol[S][W64] and the
        optional labels / violating / null bitmaps of that shape.  cap (default n_nodes) bounds
        the records; without `out` the arrays returned hold the min(cap, n_patches) records,
        with `out` they are the caller's arrays."""
        viol = np.ascontiguousarray(viol, dtype=np.uint64)
        s = viol.shape[0]
        labels, violating, null = self._bitmaps(viol.shape, labels=labels, violating=violating,
                                                null=null)
        ids = self._name_ids(names, s)
        cap = n_nodes if cap is None else cap
        node, add, rem = self._patch_records(cap, out)
        n, total = c_int64(), c_int64()
        opt = lambda m: _ptr(m) if m is not None and m.size else None  # noqa: E731
        rc = self._l.pas_tas_label_patches(self._h, n_nodes, s, opt(viol), _ptr(ids), opt(labels),
                                           opt(violating), opt(null), cap, opt(node), opt(add),
                                           opt(rem), byref(n), byref(total))
        self._check(rc, "pas_tas_label_patches")
        if out is None:
            k = min(cap, n.value)
            node, add, rem = node[:k], add[:k], rem[:k]
        return node, add, rem, n.value, total.value

    def tas_label_patches_device(self, n_nodes: int, n_strat: int, viol_t, labels_t, violating_t,
                                 null_t, cap: int, node_t, add_t, rem_t, n_patches_t, total_t,
                                 stream=None, names=None):
        ids = self._name_ids(names, n_strat)
        rc = self._l.pas_tas_label_patches_device(
            self._h, n_nodes, n_strat, _dptr(viol_t), _ptr(ids), _dptr(labels_t),
            _dptr(violating_t), _dptr(null_t), cap, _dptr(node_t), _dptr(add_t), _dptr(rem_t),
            _dptr(n_patches_t), _dptr(total_t), _stream(stream))
        self._check(rc, "pas_tas_label_patches_device")

    def tas_deschedule_patches(self, gen: int, rules: np.ndarray, rule_off: np.ndarray,
                               labels: Optional[np.ndarray] = None, names=None,
                               violating: Optional[np.ndarray] = None,
                               null: Optional[np.ndarray] = None, cap: Optional[int] = None,
                               out=None, want_viol: bool = False):
        """The sweep of tas_violations and tas_label_patches on its bitmaps in one call
        (pas_tas_deschedule_patches): (node, add, rem, n_patches, total), and the sweep's
        viol[S][W64] as a sixth item with want_viol."""
        rule_off = np.ascontiguousarray(rule_off, dtype=np.int32)
        s = rule_off.shape[0] - 1
        rules = np.ascontiguousarray(rules, dtype=RULE_DTYPE)
        n_nodes = self.n_nodes
        shape = (s, w64(n_nodes))
        labels, violating, null = self._bitmaps(shape, labels=labels, violating=violating,
                                                null=null)
        ids = self._name_ids(names, s)
        cap = n_nodes if cap is None else cap
        node, add, rem = self._patch_records(cap, out)
        viol = np.zeros(shape, np.uint64) if want_viol else None
        n, total = c_int64(), c_int64()
        opt = lambda m: _ptr(m) if m is not None and m.size else None  # noqa: E731
        rc = self._l.pas_tas_deschedule_patches(
            self._h, gen, s, opt(rules), _ptr(rule_off), _ptr(ids), opt(labels), opt(violating),
            opt(null), opt(viol), cap, opt(node), opt(add), opt(rem), byref(n), byref(total))
        self._check(rc, "pas_tas_deschedule_patches")
        if out is None:
            k = min(cap, n.value)
            node, add, rem = node[:k], add[:k], rem[:k]
        res = (node, add, rem, n.value, total.value)
        return res + (viol,) if want_viol else res

    def tas_deschedule_patches_device(self, gen: int, n_strat: int, n_rules: int, rules_t,
                                      rule_off_t, labels_t, violating_t, null_t, viol_t,
                                      cap: int, node_t, add_t, rem_t, n_patches_t, total_t,
                                      stream=None, names=None):
        """pas_tas_deschedule_patches_device: viol_t None keeps the sweep's bitmaps in the
        stream's workspace."""
        ids = self._name_ids(names, n_strat)
        rc = self._l.pas_tas_deschedule_patches_device(
            self._h, gen, n_strat, n_rules, _dptr(rules_t), _dptr(rule_off_t), _ptr(ids),
            _dptr(labels_t), _dptr(violating_t), _dptr(null_t), _dptr(viol_t), cap,
            _dptr(node_t), _dptr(add_t), _dptr(rem_t), _dptr(n_patches_t), _dptr(total_t),
            _stream(stream))
        self._check(rc, "pas_tas_deschedule_patches_device")

    # ------------------------------------------------------------------ GAS
    def gas_snapshot_set(self, gen: int, n_cards: np.ndarray, cap_per_gpu: np.ndarray,
                         used: np.ndarray):
        n_cards = np.ascontiguousarray(n_cards, dtype=np.int32)
        cap = np.ascontiguousarray(cap_per_gpu, dtype=np.int64)
        used = np.ascontiguousarray(used, dtype=np.int64)
        n, k, q = used.shape
        assert cap.shape == (n, q) and n_cards.shape == (n,)
        self._check(self._l.pas_gas_snapshot_set(self._h, gen, n, k, q, _ptr(n_cards),
                                                 _ptr(cap), _ptr(used)),
                    "pas_gas_snapshot_set")
        self.gas_shape = (n, k, q)

    def gas_snapshot_set_device(self, gen: int, n_nodes: int, max_cards: int, n_res: int,
                                n_cards_t, cap_t, used_t, stream=None):
        self._check(self._l.pas_gas_snapshot_set_device(self._h, gen, n_nodes, max_cards, n_res,
                                                        _dptr(n_cards_t), _dptr(cap_t),
                                                        _dptr(used_t), _stream(stream)),
                    "pas_gas_snapshot_set_device")
        self.gas_shape = (n_nodes, max_cards, n_res)

    def gas_fit(self, gen: int, req: np.ndarray, req_mask: np.ndarray, n_containers: np.ndarray,
                i915_index: int) -> np.ndarray:
        req = np.ascontiguousarray(req, dtype=np.int64)
        p, c, q = req.shape
        req_mask = np.ascontiguousarray(req_mask, dtype=np.uint32)
        n_containers = np.ascontiguousarray(n_containers, dtype=np.int32)
        assert req_mask.shape == (p, c) and n_containers.shape == (p,)
        out = np.zeros((p, self.gas_shape[0]), np.uint32)
        rc = self._l.pas_gas_fit(self._h, gen, p, c, i915_index, _ptr(req), _ptr(req_mask),
                                 _ptr(n_containers), _ptr(out))
        self._check(rc, "pas_gas_fit")
        return out

    def gas_fit_ex(self, gen: int, req: np.ndarray, req_mask: np.ndarray,
                   n_containers: np.ndarray, i915_index: int, side_cap: int = 1024):
        """pas_gas_fit_ex: (words [P][N], side records) — one GAS_SELECTION_DTYPE record per
        PAS_GAS_SEL_EXTENDED word (sorted by pod, node).  A side buffer that was too small is
        grown to the reported count and the call repeated."""
        req = np.ascontiguousarray(req, dtype=np.int64)
        p, c, q = req.shape
        req_mask = np.ascontiguousarray(req_mask, dtype=np.uint32)
        n_containers = np.ascontiguousarray(n_containers, dtype=np.int32)
        assert req_mask.shape == (p, c) and n_containers.shape == (p,)
        out = np.zeros((p, self.gas_shape[0]), np.uint32)
        while True:
            side = np.zeros(max(side_cap, 1), _lib.GAS_SELECTION_DTYPE)
            count = c_int64(0)
            rc = self._l.pas_gas_fit_ex(self._h, gen, p, c, i915_index, _ptr(req), _ptr(req_mask),
                                        _ptr(n_containers), _ptr(out), _ptr(side), side_cap,
                                        byref(count))
            self._check(rc, "pas_gas_fit_ex")
            if count.value <= side_cap:
                break
            side_cap = count.value
        side = side[:count.value]
        return out, side[np.lexsort((side["node"], side["pod"]))]

    def gas_fit_ex_device(self, gen: int, n_pods: int, max_containers: int, i915_index: int,
                          req_t, mask_t, ncont_t, res_t, side_t, side_cap: int, count_t,
                          stream=None):
        rc = self._l.pas_gas_fit_ex_device(self._h, gen, n_pods, max_containers, i915_index,
                                           _dptr(req_t), _dptr(mask_t), _dptr(ncont_t),
                                           _dptr(res_t), _dptr(side_t), side_cap, _dptr(count_t),
                                           _stream(stream))
        self._check(rc, "pas_gas_fit_ex_device")

    def gas_limit_count(self) -> int:
        """Pods of the last GAS fit beyond PAS_GAS_MAX_SELECTIONS (pas_gas_limit_count)."""
        v = c_int64(0)
        self._check(self._l.pas_gas_limit_count(self._h, byref(v)), "pas_gas_limit_count")
        return v.value

    def gas_bind(self, gen_from: int, gen_to: int, pods, nodes, req: np.ndarray,
                 req_mask: np.ndarray, n_containers: np.ndarray, i915_index: int,
                 selections: bool = False, counts: bool = False):
        """GASExtender.bindNode for binds (pods[b] -> nodes[b]) in order, committed into the
        resident usage.  Returns (result words, statuses), plus (cards [B][64], n_sel [B]) with
        selections=True (pas_gas_bind_ex), or plus counts [B][C][K] (selections per container
        and card, any number) with counts=True (pas_gas_bind_counts)."""
        req = np.ascontiguousarray(req, dtype=np.int64)
        p, c, q = req.shape
        req_mask = np.ascontiguousarray(req_mask, dtype=np.uint32)
        n_containers = np.ascontiguousarray(n_containers, dtype=np.int32)
        pods = np.ascontiguousarray(pods, dtype=np.int32)
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        res = np.zeros(len(pods), np.uint32)
        st = np.zeros(len(pods), np.int32)
        if counts:
            cnt = np.zeros((len(pods), c, self.gas_shape[1]), np.int64)
            rc = self._l.pas_gas_bind_counts(self._h, gen_from, gen_to, len(pods), _ptr(pods),
                                             _ptr(nodes), p, c, i915_index, _ptr(req),
                                             _ptr(req_mask), _ptr(n_containers), _ptr(res),
                                             _ptr(st), _ptr(cnt))
            self._check(rc, "pas_gas_bind_counts")
            return res, st, cnt
        if not selections:
            rc = self._l.pas_gas_bind(self._h, gen_from, gen_to, len(pods), _ptr(pods),
                                      _ptr(nodes), p, c, i915_index, _ptr(req), _ptr(req_mask),
                                      _ptr(n_containers), _ptr(res), _ptr(st))
            self._check(rc, "pas_gas_bind")
            return res, st
        cards = np.zeros((len(pods), _lib.PAS_GAS_MAX_SELECTIONS), np.uint8)
        nsel = np.zeros(len(pods), np.int32)
        rc = self._l.pas_gas_bind_ex(self._h, gen_from, gen_to, len(pods), _ptr(pods),
                                     _ptr(nodes), p, c, i915_index, _ptr(req), _ptr(req_mask),
                                     _ptr(n_containers), _ptr(res), _ptr(st), _ptr(cards),
                                     _ptr(nsel))
        self._check(rc, "pas_gas_bind_ex")
        return res, st, cards, nsel

    def gas_place(self, gen_from: int, gen_to: int, req: np.ndarray, req_mask: np.ndarray,
                  n_containers: np.ndarray, i915_index: int, cand_node, cand_len=None,
                  k: Optional[int] = None, node_base: int = 0, selections: bool = False,
                  counts: bool = False, rounds: bool = False):
        """Batch placement (pas_gas_place): pod p, in order, binds to the first node of its row
        cand_node[p, :k] (cut to cand_len[p]) that takes it on the usage the pods before it
        left.  Returns (place_node [P], place_rank [P], result words [P], n_placed), then
        (cards [P][64], n_sel [P]) with selections=True, counts [P][C][K] with counts=True and
        the number of device rounds with rounds=True, in that order."""
        req = np.ascontiguousarray(req, dtype=np.int64)
        p, c, q = req.shape
        req_mask = np.ascontiguousarray(req_mask, dtype=np.uint32)
        n_containers = np.ascontiguousarray(n_containers, dtype=np.int32)
        cand_node = np.ascontiguousarray(cand_node, dtype=np.int32)
        assert cand_node.ndim == 2 and cand_node.shape[0] == p, "cand_node is [P][ld]"
        ld = cand_node.shape[1]
        k = ld if k is None else k
        if cand_len is not None:
            cand_len = np.ascontiguousarray(cand_len, dtype=np.int32)
        node = np.zeros(p, np.int32)
        rank = np.zeros(p, np.int32)
        res = np.zeros(p, np.uint32)
        cards = np.zeros((p, _lib.PAS_GAS_MAX_SELECTIONS), np.uint8) if selections else None
        nsel = np.zeros(p, np.int32) if selections else None
        cnt = np.zeros((p, c, self.gas_shape[1]), np.int64) if counts else None
        n_placed, n_rounds = c_int32(0), c_int32(0)
        rc = self._l.pas_gas_place(self._h, gen_from, gen_to, p, c, i915_index, _ptr(req),
                                   _ptr(req_mask), _ptr(n_containers), k, ld, node_base,
                                   _ptr(cand_node), _ptr(cand_len), _ptr(node), _ptr(rank),
                                   _ptr(res), _ptr(cards), _ptr(nsel), _ptr(cnt),
                                   byref(n_placed), byref(n_rounds))
        self._check(rc, "pas_gas_place")
        out = (node, rank, res, n_placed.value)
        out += (cards, nsel) if selections else ()
        out += (cnt,) if counts else ()
        return out + ((n_rounds.value,) if rounds else ())

    def gas_place_device(self, gen_from: int, gen_to: int, n_pods: int, max_containers: int,
                         i915_index: int, req_t, mask_t, ncont_t, k: int, ld: int,
                         node_base: int, cand_t, len_t, place_node_t, place_rank_t, res_t,
                         cards_t=None, nsel_t=None, counts_t=None, stream=None):
        """pas_gas_place_device on device tensors (len_t, cards_t / nsel_t and counts_t may be
        None); returns (n_placed, device rounds) once the placement is complete."""
        n_placed, n_rounds = c_int32(0), c_int32(0)
        rc = self._l.pas_gas_place_device(
            self._h, gen_from, gen_to, n_pods, max_containers, i915_index, _dptr(req_t),
            _dptr(mask_t), _dptr(ncont_t), k, ld, node_base, _dptr(cand_t), _dptr(len_t),
            _dptr(place_node_t), _dptr(place_rank_t), _dptr(res_t), _dptr(cards_t),
            _dptr(nsel_t), _dptr(counts_t), byref(n_placed), byref(n_rounds), _stream(stream))
        self._check(rc, "pas_gas_place_device")
        return n_placed.value, n_rounds.value

    def gas_release(self, gen_from: int, gen_to: int, pods, nodes, req: np.ndarray,
                    req_mask: np.ndarray, n_containers: np.ndarray, cards_per_container,
                    cards) -> np.ndarray:
        """adjustPodResources(remove) for pods leaving nodes; returns statuses.  cards is
        [R][8] (pas_gas_release) or [R][64] (pas_gas_release_ex)."""
        req = np.ascontiguousarray(req, dtype=np.int64)
        p, c, q = req.shape
        req_mask = np.ascontiguousarray(req_mask, dtype=np.uint32)
        n_containers = np.ascontiguousarray(n_containers, dtype=np.int32)
        pods = np.ascontiguousarray(pods, dtype=np.int32)
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        cpc = np.ascontiguousarray(cards_per_container, dtype=np.int32).reshape(len(pods), c)
        cards = np.ascontiguousarray(cards, dtype=np.int32)
        ex = cards.size == len(pods) * _lib.PAS_GAS_MAX_SELECTIONS and cards.size > 0
        cards = cards.reshape(len(pods), _lib.PAS_GAS_MAX_SELECTIONS if ex else _lib.PAS_GAS_PACKED)
        st = np.zeros(len(pods), np.int32)
        fn = self._l.pas_gas_release_ex if ex else self._l.pas_gas_release
        rc = fn(self._h, gen_from, gen_to, len(pods), _ptr(pods), _ptr(nodes), p, c, _ptr(req),
                _ptr(req_mask), _ptr(n_containers), _ptr(cpc), _ptr(cards), _ptr(st))
        self._check(rc, "pas_gas_release_ex" if ex else "pas_gas_release")
        return st

    def gas_release_counts(self, gen_from: int, gen_to: int, pods, nodes, req: np.ndarray,
                           req_mask: np.ndarray, n_containers: np.ndarray,
                           counts) -> np.ndarray:
        """adjustPodResources(remove) with each annotation as counts [R][C][K] (container c
        lists card k that many times; pas_gas_release_counts); returns statuses."""
        req = np.ascontiguousarray(req, dtype=np.int64)
        p, c, q = req.shape
        req_mask = np.ascontiguousarray(req_mask, dtype=np.uint32)
        n_containers = np.ascontiguousarray(n_containers, dtype=np.int32)
        pods = np.ascontiguousarray(pods, dtype=np.int32)
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(
            len(pods), c, self.gas_shape[1])
        st = np.zeros(len(pods), np.int32)
        rc = self._l.pas_gas_release_counts(self._h, gen_from, gen_to, len(pods), _ptr(pods),
                                            _ptr(nodes), p, c, _ptr(req), _ptr(req_mask),
                                            _ptr(n_containers), _ptr(counts), _ptr(st))
        self._check(rc, "pas_gas_release_counts")
        return st

    def gas_apply(self, gen_from: int, gen_to: int, kinds, pods, nodes, req: np.ndarray,
                  req_mask: np.ndarray, n_containers: np.ndarray, cards_per_container,
                  cards) -> np.ndarray:
        """Pod events in order (pas_gas_apply): kinds[e] is PAS_GAS_EV_ADD (adjustPodResources
        (add) from the annotation: no fit, no capacity check) or PAS_GAS_EV_REMOVE
        (pas_gas_release_ex) of pod pods[e] on node nodes[e].  cards_per_container is [E][C],
        cards [E][cards_ld] with any row length cards_ld >= 1; returns statuses [E]."""
        req = np.ascontiguousarray(req, dtype=np.int64)
        p, c, q = req.shape
        req_mask = np.ascontiguousarray(req_mask, dtype=np.uint32)
        n_containers = np.ascontiguousarray(n_containers, dtype=np.int32)
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        pods = np.ascontiguousarray(pods, dtype=np.int32)
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        e = len(kinds)
        assert pods.shape == (e,) and nodes.shape == (e,)
        cpc = np.ascontiguousarray(cards_per_container, dtype=np.int32).reshape(e, c)
        cards = np.ascontiguousarray(cards, dtype=np.int32)
        assert cards.ndim == 2 and cards.shape[0] == e, "cards is [E][cards_ld]"
        st = np.zeros(e, np.int32)
        rc = self._l.pas_gas_apply(self._h, gen_from, gen_to, e, _ptr(kinds), _ptr(pods),
                                   _ptr(nodes), p, c, _ptr(req), _ptr(req_mask),
                                   _ptr(n_containers), _ptr(cpc), _ptr(cards), cards.shape[1],
                                   _ptr(st))
        self._check(rc, "pas_gas_apply")
        return st

    def gas_apply_device(self, gen_from: int, gen_to: int, n_events: int, kinds_t, pods_t,
                         nodes_t, n_pods: int, max_containers: int, req_t, mask_t, ncont_t,
                         cpc_t, cards_t, cards_ld: int, status_t, stream=None):
        """pas_gas_apply_device on device tensors: asynchronous on the stream, the statuses are
        in status_t once the stream has run."""
        rc = self._l.pas_gas_apply_device(
            self._h, gen_from, gen_to, n_events, _dptr(kinds_t), _dptr(pods_t), _dptr(nodes_t),
            n_pods, max_containers, _dptr(req_t), _dptr(mask_t), _dptr(ncont_t), _dptr(cpc_t),
            _dptr(cards_t), cards_ld, _dptr(status_t), _stream(stream))
        self._check(rc, "pas_gas_apply_device")

    # ---- pod events from annotation strings (csrc/gas_annotations.hip)
    def _pod_batch(self, req, req_mask, n_containers):
        req = np.ascontiguousarray(req, dtype=np.int64)
        assert req.ndim == 3, "req is [P][C][Q]"
        return (req, np.ascontiguousarray(req_mask, dtype=np.uint32),
                np.ascontiguousarray(n_containers, dtype=np.int32))

    def gas_apply_annotations(self, gen_from: int, gen_to: int, kinds, pods, nodes,
                              req: np.ndarray, req_mask: np.ndarray, n_containers: np.ndarray,
                              ann_off, ann_blob) -> np.ndarray:
        """Pod events in order with the annotations as strings (pas_gas_apply_annotations):
        event e is kinds[e] of pod pods[e] on node slot nodes[e] (-1: a node the snapshot does
        not hold) with the annotation ann_blob[ann_off[e]:ann_off[e + 1]] (snapshot.pack_names
        packs them); the cards are resolved against the card-name table on the device.
        Returns statuses [E], PAS_GAS_ERR_BAD_ARGS included."""
        req, req_mask, n_containers = self._pod_batch(req, req_mask, n_containers)
        p, c, _ = req.shape
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        pods = np.ascontiguousarray(pods, dtype=np.int32)
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        off, e = self._csr(ann_off)
        assert kinds.shape == (e,) and pods.shape == (e,) and nodes.shape == (e,)
        st = np.zeros(max(e, 1), np.int32)
        rc = self._l.pas_gas_apply_annotations(
            self._h, gen_from, gen_to, e, _ptr(kinds), _ptr(pods), _ptr(nodes), p, c, _ptr(req),
            _ptr(req_mask), _ptr(n_containers), _ptr(off), _ptr(self._blob(ann_blob)), _ptr(st))
        self._check(rc, "pas_gas_apply_annotations")
        return st[:e]

    def gas_apply_annotations_names(self, gen_from: int, gen_to: int, kinds, pods, node_name_off,
                                    node_name_blob, req: np.ndarray, req_mask: np.ndarray,
                                    n_containers: np.ndarray, ann_off, ann_blob) -> np.ndarray:
        """The same with each event's node given by name, resolved through the name table
        (pas_gas_apply_annotations_names): a name without a slot is an event that succeeds and
        changes nothing, an empty name PAS_GAS_ERR_BAD_ARGS."""
        req, req_mask, n_containers = self._pod_batch(req, req_mask, n_containers)
        p, c, _ = req.shape
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        pods = np.ascontiguousarray(pods, dtype=np.int32)
        off, e = self._csr(ann_off)
        n_off, e2 = self._csr(node_name_off)
        assert kinds.shape == (e,) and pods.shape == (e,) and e2 == e
        st = np.zeros(max(e, 1), np.int32)
        rc = self._l.pas_gas_apply_annotations_names(
            self._h, gen_from, gen_to, e, _ptr(kinds), _ptr(pods), _ptr(n_off),
            _ptr(self._blob(node_name_blob)), p, c, _ptr(req), _ptr(req_mask), _ptr(n_containers),
            _ptr(off), _ptr(self._blob(ann_blob)), _ptr(st))
        self._check(rc, "pas_gas_apply_annotations_names")
        return st[:e]

    def gas_apply_annotations_device(self, gen_from: int, gen_to: int, n_events: int, kinds_t,
                                     pods_t, nodes_t, n_pods: int, max_containers: int, req_t,
                                     mask_t, ncont_t, n_ann_bytes: int, ann_off_t, ann_bytes_t,
                                     status_t, stream=None):
        """pas_gas_apply_annotations_device on device tensors: synchronizes the stream once (the
        rank rows' length comes back), the statuses are in status_t once the stream has run."""
        rc = self._l.pas_gas_apply_annotations_device(
            self._h, gen_from, gen_to, n_events, _dptr(kinds_t), _dptr(pods_t), _dptr(nodes_t),
            n_pods, max_containers, _dptr(req_t), _dptr(mask_t), _dptr(ncont_t), n_ann_bytes,
            _dptr(ann_off_t), _dptr(ann_bytes_t), _dptr(status_t), _stream(stream))
        self._check(rc, "pas_gas_apply_annotations_device")

    def gas_apply_annotations_names_device(self, gen_from: int, gen_to: int, n_events: int,
                                           kinds_t, pods_t, n_name_bytes: int, name_off_t,
                                           name_bytes_t, n_pods: int, max_containers: int, req_t,
                                           mask_t, ncont_t, n_ann_bytes: int, ann_off_t,
                                           ann_bytes_t, status_t, stream=None):
        rc = self._l.pas_gas_apply_annotations_names_device(
            self._h, gen_from, gen_to, n_events, _dptr(kinds_t), _dptr(pods_t), n_name_bytes,
            _dptr(name_off_t), _dptr(name_bytes_t), n_pods, max_containers, _dptr(req_t),
            _dptr(mask_t), _dptr(ncont_t), n_ann_bytes, _dptr(ann_off_t), _dptr(ann_bytes_t),
            _dptr(status_t), _stream(stream))
        self._check(rc, "pas_gas_apply_annotations_names_device")

    def gas_annotations_resolve(self, pods, nodes, n_containers, max_containers: int, ann_off,
                                ann_blob, cards_ld: int):
        """The parse alone (pas_gas_annotations_resolve): (verdict [E], n_listed [E],
        cards_per_container [E][max_containers], cards [E][cards_ld]); verdict is the status of
        the rules that need no card name or PAS_GAS_ANN_PENDING."""
        pods = np.ascontiguousarray(pods, dtype=np.int32)
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        ncont = np.ascontiguousarray(n_containers, dtype=np.int32)
        off, e = self._csr(ann_off)
        assert pods.shape == (e,) and nodes.shape == (e,)
        c, ld = int(max_containers), int(cards_ld)
        verdict = np.zeros(max(e, 1), np.int32)
        listed = np.zeros(max(e, 1), np.int32)
        cpc = np.zeros((max(e, 1), max(c, 1)), np.int32)
        cards = np.zeros((max(e, 1), max(ld, 1)), np.int32)
        rc = self._l.pas_gas_annotations_resolve(
            self._h, e, _ptr(pods), _ptr(nodes), len(ncont), _ptr(ncont), c, _ptr(off),
            _ptr(self._blob(ann_blob)), ld, _ptr(verdict), _ptr(listed),
            _ptr(cpc.reshape(-1)[:max(e * c, 1)]), _ptr(cards))
        self._check(rc, "pas_gas_annotations_resolve")
        flat = cpc.reshape(-1)[:e * c].reshape(e, c)
        return verdict[:e], listed[:e], flat, cards[:e]

    def gas_annotations_resolve_device(self, n_events: int, pods_t, nodes_t, n_pods: int, ncont_t,
                                       max_containers: int, n_ann_bytes: int, ann_off_t,
                                       ann_bytes_t, cards_ld: int, verdict_t, listed_t, cpc_t,
                                       cards_t, stream=None):
        rc = self._l.pas_gas_annotations_resolve_device(
            self._h, n_events, _dptr(pods_t), _dptr(nodes_t), n_pods, _dptr(ncont_t),
            max_containers, n_ann_bytes, _dptr(ann_off_t), _dptr(ann_bytes_t), cards_ld,
            _dptr(verdict_t), _dptr(listed_t), _dptr(cpc_t), _dptr(cards_t), _stream(stream))
        self._check(rc, "pas_gas_annotations_resolve_device")

    # ---- bind annotations and node names rendered on the device (csrc/gas_render.hip)
    @staticmethod
    def _split_spans(raw: bytes, off, decode: bool) -> list:
        """The spans raw[off[i]:off[i + 1]] as bytes, or with decode as str (UTF-8, undecodable
        bytes as surrogate escapes)."""
        o = [int(x) for x in off]
        if decode and raw.isascii():  # byte offsets are character offsets: one decode
            raw, decode = raw.decode(), False
        out = [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]
        return [s.decode("utf-8", "surrogateescape") for s in out] if decode else out

    def _rendered(self, what: str, call, off, decode: bool) -> list:
        """The sizing call, then the call with the room it asked for."""
        total = c_int64()
        rc = call(None, 0, byref(total))
        buf = np.zeros(max(total.value, 1), np.uint8)
        if rc == _lib.PAS_ECAPACITY:
            rc = call(_ptr(buf), total.value, byref(total))
        self._check(rc, what)
        return self._split_spans(buf[:int(off[-1])].tobytes(), off, decode)

    def gas_annotations_render(self, bind_node, n_containers, counts, decode: bool = False):
        """The "gas-container-cards" values of binds given as counts [B][C][K] on node slots
        bind_node (-1: an unplaced pod), from the resident card-name table
        (pas_gas_annotations_render): (statuses [B], the B values as bytes, or as str with
        decode).  A bind whose status is not PAS_GAS_OK renders empty."""
        node = np.ascontiguousarray(bind_node, dtype=np.int32).reshape(-1)
        ncont = np.ascontiguousarray(n_containers, dtype=np.int32).reshape(-1)
        b, k = len(node), self.gas_shape[1]
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        assert len(ncont) == b and counts.size % max(b * k, 1) == 0, "counts is [B][C][K]"
        c = counts.size // (b * k) if b else 0
        status = np.zeros(max(b, 1), np.int32)
        off = np.zeros(b + 1, np.int64)

        def call(buf, cap, total):
            return self._l.pas_gas_annotations_render(
                self._h, b, _ptr(node), _ptr(ncont), c, _ptr(counts.reshape(-1)), _ptr(status),
                _ptr(off), buf, cap, total)
        return status[:b], self._rendered("pas_gas_annotations_render", call, off, decode)

    def gas_annotations_render_ranks(self, bind_node, n_containers, cards_per_container, cards,
                                     decode: bool = False):
        """The same from cards_per_container [B][C] and the containers' card ranks, consecutive
        in cards [B][cards_ld]: the arrays gas_annotations_resolve returns
        (pas_gas_annotations_render_ranks)."""
        node = np.ascontiguousarray(bind_node, dtype=np.int32).reshape(-1)
        ncont = np.ascontiguousarray(n_containers, dtype=np.int32).reshape(-1)
        b = len(node)
        cpc = np.ascontiguousarray(cards_per_container, dtype=np.int32).reshape(b, -1 if b else 0)
        cards = np.ascontiguousarray(cards, dtype=np.int32).reshape(b, -1 if b else 0)
        status = np.zeros(max(b, 1), np.int32)
        off = np.zeros(b + 1, np.int64)

        def call(buf, cap, total):
            return self._l.pas_gas_annotations_render_ranks(
                self._h, b, _ptr(node), _ptr(ncont), cpc.shape[1] if b else 0,
                _ptr(cpc.reshape(-1)), _ptr(cards.reshape(-1)), cards.shape[1] if b else 0,
                _ptr(status), _ptr(off), buf, cap, total)
        return status[:b], self._rendered("pas_gas_annotations_render_ranks", call, off, decode)

    def _render_device(self, fn, what: str, head, status_t, off_t, bytes_t, cap: int, stream):
        total = c_int64()
        rc = fn(self._h, *head, *((_dptr(status_t),) if status_t is not None else ()),
                _dptr(off_t), _dptr(bytes_t), cap, byref(total), _stream(stream))
        if rc != _lib.PAS_OK:
            msg = self._l.pas_last_error(self._h)
            err = PasError(rc, f"{what}: {msg.decode() if msg else ''}")
            err.n_bytes = total.value  # PAS_ECAPACITY: the room the bytes need
            raise err
        return total.value

    def gas_annotations_render_device(self, n_binds: int, bind_node_t, ncont_t,
                                      max_containers: int, counts_t, status_t, ann_off_t,
                                      ann_bytes_t, cap: int, stream=None) -> int:
        """pas_gas_annotations_render_device on device tensors; returns the byte total.  The
        stream is synchronized once; a short cap (0 with ann_bytes_t None: the sizing call)
        raises PasError(PAS_ECAPACITY) with the total in err.n_bytes and the statuses and
        offsets delivered."""
        return self._render_device(
            self._l.pas_gas_annotations_render_device, "pas_gas_annotations_render_device",
            (n_binds, _dptr(bind_node_t), _dptr(ncont_t), max_containers, _dptr(counts_t)),
            status_t, ann_off_t, ann_bytes_t, cap, stream)

    def gas_annotations_render_ranks_device(self, n_binds: int, bind_node_t, ncont_t,
                                            max_containers: int, cpc_t, cards_t, cards_ld: int,
                                            status_t, ann_off_t, ann_bytes_t, cap: int,
                                            stream=None) -> int:
        return self._render_device(
            self._l.pas_gas_annotations_render_ranks_device,
            "pas_gas_annotations_render_ranks_device",
            (n_binds, _dptr(bind_node_t), _dptr(ncont_t), max_containers, _dptr(cpc_t),
             _dptr(cards_t), cards_ld), status_t, ann_off_t, ann_bytes_t, cap, stream)

    def names_render(self, slots, slot_base: int = 0, decode: bool = False) -> list:
        """The names of the node slots slots[i] - slot_base from the resident name table
        (pas_names_render), as bytes or with decode as str; a spare slot or one outside the
        table, -1 included, gives the empty name."""
        slot = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        off = np.zeros(len(slot) + 1, np.int64)

        def call(buf, cap, total):
            return self._l.pas_names_render(self._h, len(slot),
                                            _ptr(slot) if slot.size else None, slot_base,
                                            _ptr(off), buf, cap, total)
        return self._rendered("pas_names_render", call, off, decode)

    def names_render_device(self, n: int, slot_t, slot_base: int, off_t, bytes_t, cap: int,
                            stream=None) -> int:
        """pas_names_render_device on device tensors; returns the byte total (short cap: as
        gas_annotations_render_device)."""
        return self._render_device(self._l.pas_names_render_device, "pas_names_render_device",
                                   (n, _dptr(slot_t), slot_base), None, off_t, bytes_t, cap,
                                   stream)

    # ---- the resident card-name table (csrc/gas_cards.hip)
    def gas_card_names_set(self, n_slots: int, k: int, name_off, blob):
        """Install the card-name table (pas_gas_card_names_set): n_slots rows of k names, name
        (s, c) = blob[name_off[s * k + c]:name_off[s * k + c + 1]] (snapshot.pack_card_names)."""
        off, n = self._csr(name_off)
        assert n == n_slots * k, "name_off holds n_slots * k + 1 entries"
        self._check(self._l.pas_gas_card_names_set(self._h, n_slots, k, _ptr(off),
                                                   _ptr(self._blob(blob))),
                    "pas_gas_card_names_set")

    def gas_card_names_update(self, row_slot, name_off, blob):
        """Rewrite whole rows in call order (pas_gas_card_names_update): row r of name_off /
        blob replaces slot row_slot[r]; a slot given twice keeps the later row."""
        rows = np.ascontiguousarray(row_slot, dtype=np.int32).reshape(-1)
        off, _ = self._csr(name_off)
        self._check(self._l.pas_gas_card_names_update(
            self._h, len(rows), _ptr(rows) if rows.size else None, _ptr(off),
            _ptr(self._blob(blob))), "pas_gas_card_names_update")

    def gas_card_names_resize(self, n_slots: int, k: int, stream=None):
        self._check(self._l.pas_gas_card_names_resize(self._h, n_slots, k, _stream(stream)),
                    "pas_gas_card_names_resize")

    def gas_card_names_remap(self, src_slot, stream=None):
        """Renumber the table's rows with a compact map (pas_gas_card_names_remap)."""
        src = np.ascontiguousarray(src_slot, dtype=np.int32).reshape(-1)
        self._check(self._l.pas_gas_card_names_remap(
            self._h, len(src), _ptr(src) if src.size else None, _stream(stream)),
            "pas_gas_card_names_remap")

    def gas_card_names_info(self):
        """(n_slots, k, n_bytes) of the card-name table; n_bytes counts the pool's dead bytes
        too."""
        n, k, b = c_int32(), c_int32(), c_int64()
        self._check(self._l.pas_gas_card_names_info(self._h, byref(n), byref(k), byref(b)),
                    "pas_gas_card_names_info")
        return n.value, k.value, b.value

    def gas_card_names_get(self):
        """(name_off int64 [n_slots * k + 1], blob bytes): the names packed in (slot, card)
        order."""
        n, k, nb = self.gas_card_names_info()
        off = np.zeros(n * k + 1, np.int64)
        buf = np.zeros(max(nb, 1), np.uint8)
        self._check(self._l.pas_gas_card_names_get(self._h, _ptr(off), _ptr(buf), nb),
                    "pas_gas_card_names_get")
        return off, buf[:int(off[-1])].tobytes()

    def gas_card_names_get_rows(self, row_slot, decode: bool = False) -> List[list]:
        """The names of the rows row_slot alone (pas_gas_card_names_get_rows): per row its k
        names in slot order, as bytes, or with decode as str (UTF-8, undecodable bytes as
        surrogate escapes)."""
        rows = np.ascontiguousarray(row_slot, dtype=np.int32).reshape(-1)
        _, k, nb = self.gas_card_names_info()
        off = np.zeros(len(rows) * k + 1, np.int64)
        buf = np.zeros(max(nb, 1), np.uint8)
        rc = self._l.pas_gas_card_names_get_rows(
            self._h, len(rows), _ptr(rows) if rows.size else None, _ptr(off), _ptr(buf), nb)
        if rc == _lib.PAS_ECAPACITY:  # (rows repeated past the pool's size)
            buf = np.zeros(int(off[-1]), np.uint8)
            rc = self._l.pas_gas_card_names_get_rows(self._h, len(rows), _ptr(rows), _ptr(off),
                                                     _ptr(buf), len(buf))
        self._check(rc, "pas_gas_card_names_get_rows")
        raw, o = buf[:int(off[-1])].tobytes(), off.tolist()
        if decode and raw.isascii():  # byte offsets are character offsets: one decode
            raw = raw.decode()
            decode = False
        out = [[raw[o[i]:o[i + 1]] for i in range(r * k, r * k + k)] for r in range(len(rows))]
        if decode:
            out = [[c.decode("utf-8", "surrogateescape") for c in row] for row in out]
        return out

    def gas_card_names_drop(self):
        self._check(self._l.pas_gas_card_names_drop(self._h), "pas_gas_card_names_drop")

    def gas_snapshot_get(self):
        """(generation, used [N][K][Q]) of the resident GAS snapshot."""
        n, k, q = self.gas_shape
        used = np.zeros((n, k, q), np.int64)
        g = c_uint64()
        self._check(self._l.pas_gas_snapshot_get(self._h, byref(g), _ptr(used)),
                    "pas_gas_snapshot_get")
        return g.value, used

    def gas_snapshot_info(self):
        """(generation, n_nodes, max_cards, n_res) of the resident GAS snapshot."""
        g, n, k, q = c_uint64(), c_int32(), c_int32(), c_int32()
        self._check(self._l.pas_gas_snapshot_info(self._h, byref(g), byref(n), byref(k),
                                                  byref(q)), "pas_gas_snapshot_info")
        return g.value, n.value, k.value, q.value

    def gas_snapshot_get_nodes(self):
        """(generation, n_cards [N], cap [N][Q]) of the resident GAS snapshot."""
        n, _, q = self.gas_shape
        n_cards = np.zeros(n, np.int32)
        cap = np.zeros((n, q), np.int64)
        g = c_uint64()
        self._check(self._l.pas_gas_snapshot_get_nodes(self._h, byref(g), _ptr(n_cards),
                                                       _ptr(cap)), "pas_gas_snapshot_get_nodes")
        return g.value, n_cards, cap

    def gas_nodes_update(self, gen_from: int, gen_to: int, nodes, n_cards, cap, src) -> np.ndarray:
        """Node events in order (pas_gas_nodes_update): update u gives node slot nodes[u] the
        card count n_cards[u], the capacities cap[u] [Q] and the usage row gathered through
        src[u] [max_cards] (slot k takes the old slot src[u][k], zeros for a negative one);
        returns statuses [U]."""
        n, k, q = self.gas_shape
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        u = len(nodes)
        n_cards = np.ascontiguousarray(n_cards, dtype=np.int32)
        cap = np.ascontiguousarray(cap, dtype=np.int64).reshape(u, q)
        src = np.ascontiguousarray(src, dtype=np.int32).reshape(u, k)
        assert n_cards.shape == (u,)
        st = np.zeros(u, np.int32)
        rc = self._l.pas_gas_nodes_update(self._h, gen_from, gen_to, u, _ptr(nodes),
                                          _ptr(n_cards), _ptr(cap), _ptr(src), _ptr(st))
        self._check(rc, "pas_gas_nodes_update")
        return st

    def _node_strings(self, u, states, label_off, cap_off):
        q = self.gas_shape[2]
        states = np.ascontiguousarray(states, dtype=np.int32).reshape(-1)
        l_off, u2 = self._csr(label_off)
        c_off, uq = self._csr(cap_off)
        assert states.shape == (u,) and u2 == u and uq == u * q, \
            "one state and label per update, n_res literals per update"
        return states, l_off, c_off

    def _nodes_update_strings(self, fn, gen_from, gen_to, u, head, states, label_off, label_blob,
                              cap_off, cap_blob):
        q = self.gas_shape[2]
        states, l_off, c_off = self._node_strings(u, states, label_off, cap_off)
        st = np.zeros(max(u, 1), np.int32)
        n_cards = np.zeros(max(u, 1), np.int32)
        cap = np.zeros((max(u, 1), max(q, 1)), np.int64)
        dropped = np.zeros(max(u, 1), np.int32)
        need = c_int32()
        rc = getattr(self._l, fn)(
            self._h, gen_from, gen_to, u, *head, _ptr(states), _ptr(l_off),
            _ptr(self._blob(label_blob)), _ptr(c_off), _ptr(self._blob(cap_blob)), _ptr(st),
            _ptr(n_cards), _ptr(cap.reshape(-1)[:max(u * q, 1)]), _ptr(dropped), byref(need))
        if rc == _lib.PAS_ECAPACITY:
            e = PasError(rc, f"{fn}: {self.last_error()}")
            e.need_cards = need.value
            raise e
        self._check(rc, fn)
        return st[:u], n_cards[:u], cap.reshape(-1)[:u * q].reshape(u, q), dropped[:u]

    def gas_nodes_update_strings(self, gen_from: int, gen_to: int, nodes, states, label_off,
                                 label_blob, cap_off, cap_blob):
        """Node events from strings (pas_gas_nodes_update_strings): update u gives node slot
        nodes[u] the state states[u] (PAS_GAS_NODE_GONE / NO_LABEL / LABEL), the cards label
        label_blob[label_off[u]:label_off[u + 1]] and one allocatable literal per resource kind,
        cap_blob[cap_off[u * Q + q]:...] (snapshot.pack_node_strings).  Returns (status [U],
        n_cards [U], cap [U][Q], n_dropped [U]).  PasError(PAS_ECAPACITY) carries need_cards, the
        largest distinct card count: nothing has changed, grow by a tier and call again."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        return self._nodes_update_strings("pas_gas_nodes_update_strings", gen_from, gen_to,
                                          len(nodes), (_ptr(nodes) if nodes.size else None,),
                                          states, label_off, label_blob, cap_off, cap_blob)

    def gas_nodes_update_strings_names(self, gen_from: int, gen_to: int, node_name_off,
                                       node_name_blob, states, label_off, label_blob, cap_off,
                                       cap_blob):
        """The same with each update's node given by name, resolved through the name table
        (pas_gas_nodes_update_strings_names): first-seen nodes take their slots through
        names_assign beforehand."""
        n_off, u = self._csr(node_name_off)
        return self._nodes_update_strings("pas_gas_nodes_update_strings_names", gen_from, gen_to,
                                          u, (_ptr(n_off), _ptr(self._blob(node_name_blob))),
                                          states, label_off, label_blob, cap_off, cap_blob)

    def gas_nodes_resolve_strings(self, nodes, states, label_off, label_blob, cap_off, cap_blob):
        """The parse and the resolve alone (pas_gas_nodes_resolve_strings), nothing resident
        written: (status [U], n_cards [U], gpu_count [U], cap [U][Q], src [U][max_cards],
        n_dropped [U])."""
        _, k, q = self.gas_shape
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        u = len(nodes)
        states, l_off, c_off = self._node_strings(u, states, label_off, cap_off)
        st, n_cards, gpus, dropped = (np.zeros(max(u, 1), np.int32) for _ in range(4))
        cap = np.zeros(max(u * q, 1), np.int64)
        src = np.zeros(max(u * k, 1), np.int32)
        rc = self._l.pas_gas_nodes_resolve_strings(
            self._h, u, _ptr(nodes) if nodes.size else None, _ptr(states), _ptr(l_off),
            _ptr(self._blob(label_blob)), _ptr(c_off), _ptr(self._blob(cap_blob)), _ptr(st),
            _ptr(n_cards), _ptr(gpus), _ptr(cap), _ptr(src), _ptr(dropped))
        self._check(rc, "pas_gas_nodes_resolve_strings")
        return (st[:u], n_cards[:u], gpus[:u], cap[:u * q].reshape(u, q),
                src[:u * k].reshape(u, k), dropped[:u])

    def gas_nodes_update_strings_device(self, gen_from: int, gen_to: int, n_updates: int, nodes_t,
                                        states_t, n_label_bytes: int, label_off_t, label_bytes_t,
                                        n_cap_bytes: int, cap_off_t, cap_bytes_t, status_t,
                                        n_cards_t=None, cap_t=None, dropped_t=None,
                                        stream=None) -> int:
        """pas_gas_nodes_update_strings_device on device tensors: synchronizes the stream once
        per run position (once for a batch without a repeated node); returns need_cards.
        PasError(PAS_ECAPACITY) carries need_cards too."""
        need = c_int32()
        rc = self._l.pas_gas_nodes_update_strings_device(
            self._h, gen_from, gen_to, n_updates, _dptr(nodes_t), _dptr(states_t), n_label_bytes,
            _dptr(label_off_t), _dptr(label_bytes_t), n_cap_bytes, _dptr(cap_off_t),
            _dptr(cap_bytes_t), _dptr(status_t), _dptr(n_cards_t), _dptr(cap_t),
            _dptr(dropped_t), byref(need), _stream(stream))
        if rc == _lib.PAS_ECAPACITY:
            e = PasError(rc, f"pas_gas_nodes_update_strings_device: {self.last_error()}")
            e.need_cards = need.value
            raise e
        self._check(rc, "pas_gas_nodes_update_strings_device")
        return need.value

    def gas_nodes_update_strings_names_device(self, gen_from: int, gen_to: int, n_updates: int,
                                              n_name_bytes: int, name_off_t, name_bytes_t,
                                              states_t, n_label_bytes: int, label_off_t,
                                              label_bytes_t, n_cap_bytes: int, cap_off_t,
                                              cap_bytes_t, status_t, n_cards_t=None, cap_t=None,
                                              dropped_t=None, stream=None) -> int:
        need = c_int32()
        rc = self._l.pas_gas_nodes_update_strings_names_device(
            self._h, gen_from, gen_to, n_updates, n_name_bytes, _dptr(name_off_t),
            _dptr(name_bytes_t), _dptr(states_t), n_label_bytes, _dptr(label_off_t),
            _dptr(label_bytes_t), n_cap_bytes, _dptr(cap_off_t), _dptr(cap_bytes_t),
            _dptr(status_t), _dptr(n_cards_t), _dptr(cap_t), _dptr(dropped_t), byref(need),
            _stream(stream))
        if rc == _lib.PAS_ECAPACITY:
            e = PasError(rc, f"pas_gas_nodes_update_strings_names_device: {self.last_error()}")
            e.need_cards = need.value
            raise e
        self._check(rc, "pas_gas_nodes_update_strings_names_device")
        return need.value

    def gas_nodes_resolve_strings_device(self, n_updates: int, nodes_t, states_t,
                                         n_label_bytes: int, label_off_t, label_bytes_t,
                                         n_cap_bytes: int, cap_off_t, cap_bytes_t, status_t,
                                         n_cards_t=None, gpus_t=None, cap_t=None, src_t=None,
                                         dropped_t=None, stream=None):
        rc = self._l.pas_gas_nodes_resolve_strings_device(
            self._h, n_updates, _dptr(nodes_t), _dptr(states_t), n_label_bytes,
            _dptr(label_off_t), _dptr(label_bytes_t), n_cap_bytes, _dptr(cap_off_t),
            _dptr(cap_bytes_t), _dptr(status_t), _dptr(n_cards_t), _dptr(gpus_t), _dptr(cap_t),
            _dptr(src_t), _dptr(dropped_t), _stream(stream))
        self._check(rc, "pas_gas_nodes_resolve_strings_device")

    def gas_nodes_update_device(self, gen_from: int, gen_to: int, n_updates: int, nodes_t,
                                n_cards_t, cap_t, src_t, status_t, stream=None):
        """pas_gas_nodes_update_device on device tensors: asynchronous on the stream, the
        statuses are in status_t once the stream has run."""
        rc = self._l.pas_gas_nodes_update_device(
            self._h, gen_from, gen_to, n_updates, _dptr(nodes_t), _dptr(n_cards_t),
            _dptr(cap_t), _dptr(src_t), _dptr(status_t), _stream(stream))
        self._check(rc, "pas_gas_nodes_update_device")

    def gas_snapshot_resize(self, gen_from: int, gen_to: int, n_nodes: int, max_cards: int,
                            stream=None):
        """Grow the resident GAS snapshot on the device (pas_gas_snapshot_resize); gas_shape
        follows."""
        self._check(self._l.pas_gas_snapshot_resize(self._h, gen_from, gen_to, n_nodes,
                                                    max_cards, _stream(stream)),
                    "pas_gas_snapshot_resize")
        self.gas_shape = (n_nodes, max_cards, self.gas_shape[2])

    def gas_snapshot_compact(self, gen_from: int, gen_to: int, src_node, stream=None):
        """Renumber the node rows of the resident GAS snapshot on the device
        (pas_gas_snapshot_compact): new row j is old row src_node[j], or a spare row for -1;
        gas_shape follows."""
        src = np.ascontiguousarray(src_node, dtype=np.int32).reshape(-1)
        self._check(self._l.pas_gas_snapshot_compact(
            self._h, gen_from, gen_to, len(src), _ptr(src) if src.size else None,
            _stream(stream)), "pas_gas_snapshot_compact")
        self.gas_shape = (len(src),) + tuple(self.gas_shape[1:])

    def gas_fit_device(self, gen: int, n_pods: int, max_containers: int, i915_index: int, req_t,
                       mask_t, ncont_t, res_t, stream=None):
        rc = self._l.pas_gas_fit_device(self._h, gen, n_pods, max_containers, i915_index,
                                        _dptr(req_t), _dptr(mask_t), _dptr(ncont_t),
                                        _dptr(res_t), _stream(stream))
        self._check(rc, "pas_gas_fit_device")

    def gas_fit_ld_device(self, gen: int, n_pods: int, max_containers: int, i915_index: int,
                          req_t, mask_t, ncont_t, res_t, ld_res: int, side_t=None,
                          side_cap: int = 0, count_t=None, stream=None):
        """pas_gas_fit_ld_device: words of (pod p, node n) at res_t.view(-1)[p * ld_res + n]."""
        rc = self._l.pas_gas_fit_ld_device(self._h, gen, n_pods, max_containers, i915_index,
                                           _dptr(req_t), _dptr(mask_t), _dptr(ncont_t),
                                           _dptr(res_t), ld_res,
                                           _dptr(side_t) if side_t is not None else None,
                                           side_cap,
                                           _dptr(count_t) if count_t is not None else None,
                                           _stream(stream))
        self._check(rc, "pas_gas_fit_ld_device")

    def gas_fit_bitmap_device(self, gen: int, n_pods: int, max_containers: int, i915_index: int,
                              req_t, mask_t, ncont_t, fit_t, stream=None):
        """GAS fit verdicts as node bitmaps fit_t[n_pods][W64] (pas_gas_fit_bitmap_device)."""
        rc = self._l.pas_gas_fit_bitmap_device(self._h, gen, n_pods, max_containers, i915_index,
                                               _dptr(req_t), _dptr(mask_t), _dptr(ncont_t),
                                               _dptr(fit_t), _stream(stream))
        self._check(rc, "pas_gas_fit_bitmap_device")

    # ------------------------------------------------------------------ node shards
    def tas_topk_device(self, gen: int, n_pods: int, n_rules: int, rules_t, rule_off_t, prio_t,
                        cand_t, k: int, node_base: int, key_t, node_t, len_t, stream=None):
        """First k HostPriorityList entries of this node shard as merge records
        (pas_tas_topk_device): key_t int64 [P][k], node_t int32 [P][k], len_t int32 [P]."""
        rc = self._l.pas_tas_topk_device(self._h, gen, n_pods, n_rules, _dptr(rules_t),
                                         _dptr(rule_off_t), _dptr(prio_t), _dptr(cand_t), k,
                                         node_base, _dptr(key_t), _dptr(node_t), _dptr(len_t),
                                         _stream(stream))
        self._check(rc, "pas_tas_topk_device")

    def tas_gas_topk_device(self, tas_gen: int, gas_gen: int, n_pods: int, n_rules: int, rules_t,
                            rule_off_t, prio_t, cand_t, max_containers: int, i915_index: int,
                            req_t, mask_t, ncont_t, k: int, node_base: int, key_t, node_t, len_t,
                            stream=None):
        """The same records over the nodes that pass TAS and fit the pod's GPU request
        (pas_tas_gas_topk_device: evaluated along each pod's order until k are kept)."""
        rc = self._l.pas_tas_gas_topk_device(
            self._h, tas_gen, gas_gen, n_pods, n_rules, _dptr(rules_t), _dptr(rule_off_t),
            _dptr(prio_t), _dptr(cand_t), max_containers, i915_index, _dptr(req_t),
            _dptr(mask_t), _dptr(ncont_t), k, node_base, _dptr(key_t), _dptr(node_t),
            _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_gas_topk_device")

    def topk_merge_device(self, n_pods: int, k: int, n_shards: int, keys_t, nodes_t, out_node_t,
                          out_len_t, stream=None):
        """Merge of [n_shards][P][k] records into the global first-k lists."""
        rc = self._l.pas_topk_merge_device(self._h, n_pods, k, n_shards, _dptr(keys_t),
                                           _dptr(nodes_t), _dptr(out_node_t), _dptr(out_len_t),
                                           _stream(stream))
        self._check(rc, "pas_topk_merge_device")

    def list_merge_device(self, n_pods: int, n_shards: int, width: int, keys_t, nodes_t,
                          out_node_t, out_len_t, out_ld: int = 0, stream=None):
        """Merge of [n_shards][P][width] whole-shard records (pas_tas_topk_device with
        k = width) into the cluster's full lists out_node [P][>= n_shards * width]."""
        out_ld = out_ld or n_shards * width
        rc = self._l.pas_list_merge_device(self._h, n_pods, n_shards, width, _dptr(keys_t),
                                           _dptr(nodes_t), _dptr(out_node_t), out_ld,
                                           _dptr(out_len_t), _stream(stream))
        self._check(rc, "pas_list_merge_device")

    # ------------------------------------------------------------------ wide merge records
    def tas_topk_wide_device(self, gen: int, n_pods: int, n_rules: int, rules_t, rule_off_t,
                             prio_t, cand_t, k: int, node_base: int, key_t, sub_t, node_t, len_t,
                             stream=None):
        """tas_topk_device with wide records (pas_tas_topk_wide_device): key_t int64 [P][k],
        sub_t uint32-sized [P][k] (torch.int32 storage), node_t int32 [P][k], len_t int32 [P];
        exact on snapshots with wide columns and across shards of different column forms."""
        rc = self._l.pas_tas_topk_wide_device(self._h, gen, n_pods, n_rules, _dptr(rules_t),
                                              _dptr(rule_off_t), _dptr(prio_t), _dptr(cand_t), k,
                                              node_base, _dptr(key_t), _dptr(sub_t),
                                              _dptr(node_t), _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_topk_wide_device")

    def tas_gas_topk_wide_device(self, tas_gen: int, gas_gen: int, n_pods: int, n_rules: int,
                                 rules_t, rule_off_t, prio_t, cand_t, max_containers: int,
                                 i915_index: int, req_t, mask_t, ncont_t, k: int, node_base: int,
                                 key_t, sub_t, node_t, len_t, stream=None):
        """tas_gas_topk_device with wide records (pas_tas_gas_topk_wide_device)."""
        rc = self._l.pas_tas_gas_topk_wide_device(
            self._h, tas_gen, gas_gen, n_pods, n_rules, _dptr(rules_t), _dptr(rule_off_t),
            _dptr(prio_t), _dptr(cand_t), max_containers, i915_index, _dptr(req_t),
            _dptr(mask_t), _dptr(ncont_t), k, node_base, _dptr(key_t), _dptr(sub_t),
            _dptr(node_t), _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_gas_topk_wide_device")

    # ------------------------------------------------------------------ resumed lists
    def tas_gas_topk_after_device(self, tas_gen: int, gas_gen: int, n_pods: int, n_rules: int,
                                  rules_t, rule_off_t, prio_t, cand_t, max_containers: int,
                                  i915_index: int, req_t, mask_t, ncont_t, k: int,
                                  node_base: int, after_key_t, after_node_t, key_t, node_t,
                                  len_t, stream=None):
        """tas_gas_topk_device resumed strictly after each pod's cursor record
        (pas_tas_gas_topk_after_device): after_key_t int64 [P], after_node_t int32 [P], global
        node ids; (INT64_MIN, -1) is the whole list, the padding record the empty list."""
        rc = self._l.pas_tas_gas_topk_after_device(
            self._h, tas_gen, gas_gen, n_pods, n_rules, _dptr(rules_t), _dptr(rule_off_t),
            _dptr(prio_t), _dptr(cand_t), max_containers, i915_index, _dptr(req_t),
            _dptr(mask_t), _dptr(ncont_t), k, node_base, _dptr(after_key_t),
            _dptr(after_node_t), _dptr(key_t), _dptr(node_t), _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_gas_topk_after_device")

    def tas_gas_topk_wide_after_device(self, tas_gen: int, gas_gen: int, n_pods: int,
                                       n_rules: int, rules_t, rule_off_t, prio_t, cand_t,
                                       max_containers: int, i915_index: int, req_t, mask_t,
                                       ncont_t, k: int, node_base: int, after_key_t, after_sub_t,
                                       after_node_t, key_t, sub_t, node_t, len_t, stream=None):
        """tas_gas_topk_wide_device resumed strictly after each pod's cursor record
        (pas_tas_gas_topk_wide_after_device): after_sub_t uint32-sized [P] (torch.int32
        storage) beside the two arrays of tas_gas_topk_after_device."""
        rc = self._l.pas_tas_gas_topk_wide_after_device(
            self._h, tas_gen, gas_gen, n_pods, n_rules, _dptr(rules_t), _dptr(rule_off_t),
            _dptr(prio_t), _dptr(cand_t), max_containers, i915_index, _dptr(req_t),
            _dptr(mask_t), _dptr(ncont_t), k, node_base, _dptr(after_key_t), _dptr(after_sub_t),
            _dptr(after_node_t), _dptr(key_t), _dptr(sub_t), _dptr(node_t), _dptr(len_t),
            _stream(stream))
        self._check(rc, "pas_tas_gas_topk_wide_after_device")

    def topk_merge_wide_device(self, n_pods: int, k: int, n_shards: int, keys_t, subs_t, nodes_t,
                               out_node_t, out_len_t, stream=None):
        """Merge of [n_shards][P][k] wide records into the global first-k lists
        (n_shards * k <= 4096)."""
        rc = self._l.pas_topk_merge_wide_device(self._h, n_pods, k, n_shards, _dptr(keys_t),
                                                _dptr(subs_t), _dptr(nodes_t),
                                                _dptr(out_node_t), _dptr(out_len_t),
                                                _stream(stream))
        self._check(rc, "pas_topk_merge_wide_device")

    def list_merge_wide_device(self, n_pods: int, n_shards: int, width: int, keys_t, subs_t,
                               nodes_t, out_node_t, out_len_t, out_ld: int = 0, stream=None):
        """Merge of [n_shards][P][width] whole-shard wide records (tas_topk_wide_device with
        k = width) into the cluster's full lists out_node [P][>= n_shards * width]."""
        out_ld = out_ld or n_shards * width
        rc = self._l.pas_list_merge_wide_device(self._h, n_pods, n_shards, width, _dptr(keys_t),
                                                _dptr(subs_t), _dptr(nodes_t),
                                                _dptr(out_node_t), out_ld, _dptr(out_len_t),
                                                _stream(stream))
        self._check(rc, "pas_list_merge_wide_device")

    # ------------------------------------------------------------------ top-k by policy id
    def tas_topk_policies_device(self, gen: int, n_pods: int, pod_policy_t, cand_t, k: int,
                                 node_base: int, key_t, node_t, len_t, stream=None):
        """tas_topk_device with pod p's rules and prio being row pod_policy_t[p] (int32 [P]) of
        the resident policy table (pas_tas_topk_policies_device); -1 = the empty list."""
        rc = self._l.pas_tas_topk_policies_device(
            self._h, gen, n_pods, _dptr(pod_policy_t), _dptr(cand_t), k, node_base,
            _dptr(key_t), _dptr(node_t), _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_topk_policies_device")

    def tas_topk_policies_wide_device(self, gen: int, n_pods: int, pod_policy_t, cand_t, k: int,
                                      node_base: int, key_t, sub_t, node_t, len_t, stream=None):
        """tas_topk_wide_device by policy id (pas_tas_topk_policies_wide_device)."""
        rc = self._l.pas_tas_topk_policies_wide_device(
            self._h, gen, n_pods, _dptr(pod_policy_t), _dptr(cand_t), k, node_base,
            _dptr(key_t), _dptr(sub_t), _dptr(node_t), _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_topk_policies_wide_device")

    def tas_gas_topk_policies_device(self, tas_gen: int, gas_gen: int, n_pods: int, pod_policy_t,
                                     cand_t, max_containers: int, i915_index: int, req_t, mask_t,
                                     ncont_t, k: int, node_base: int, key_t, node_t, len_t,
                                     stream=None):
        """tas_gas_topk_device by policy id (pas_tas_gas_topk_policies_device): a node's
        dontschedule verdict is one bit of the policy's cached violating set."""
        rc = self._l.pas_tas_gas_topk_policies_device(
            self._h, tas_gen, gas_gen, n_pods, _dptr(pod_policy_t), _dptr(cand_t),
            max_containers, i915_index, _dptr(req_t), _dptr(mask_t), _dptr(ncont_t), k,
            node_base, _dptr(key_t), _dptr(node_t), _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_gas_topk_policies_device")

    def tas_gas_topk_policies_wide_device(self, tas_gen: int, gas_gen: int, n_pods: int,
                                          pod_policy_t, cand_t, max_containers: int,
                                          i915_index: int, req_t, mask_t, ncont_t, k: int,
                                          node_base: int, key_t, sub_t, node_t, len_t,
                                          stream=None):
        """tas_gas_topk_wide_device by policy id (pas_tas_gas_topk_policies_wide_device)."""
        rc = self._l.pas_tas_gas_topk_policies_wide_device(
            self._h, tas_gen, gas_gen, n_pods, _dptr(pod_policy_t), _dptr(cand_t),
            max_containers, i915_index, _dptr(req_t), _dptr(mask_t), _dptr(ncont_t), k,
            node_base, _dptr(key_t), _dptr(sub_t), _dptr(node_t), _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_gas_topk_policies_wide_device")

    def tas_gas_topk_policies_after_device(self, tas_gen: int, gas_gen: int, n_pods: int,
                                           pod_policy_t, cand_t, max_containers: int,
                                           i915_index: int, req_t, mask_t, ncont_t, k: int,
                                           node_base: int, after_key_t, after_node_t, key_t,
                                           node_t, len_t, stream=None):
        """tas_gas_topk_after_device by policy id (pas_tas_gas_topk_policies_after_device)."""
        rc = self._l.pas_tas_gas_topk_policies_after_device(
            self._h, tas_gen, gas_gen, n_pods, _dptr(pod_policy_t), _dptr(cand_t),
            max_containers, i915_index, _dptr(req_t), _dptr(mask_t), _dptr(ncont_t), k,
            node_base, _dptr(after_key_t), _dptr(after_node_t), _dptr(key_t), _dptr(node_t),
            _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_gas_topk_policies_after_device")

    def tas_gas_topk_policies_wide_after_device(self, tas_gen: int, gas_gen: int, n_pods: int,
                                                pod_policy_t, cand_t, max_containers: int,
                                                i915_index: int, req_t, mask_t, ncont_t, k: int,
                                                node_base: int, after_key_t, after_sub_t,
                                                after_node_t, key_t, sub_t, node_t, len_t,
                                                stream=None):
        """tas_gas_topk_wide_after_device by policy id
        (pas_tas_gas_topk_policies_wide_after_device)."""
        rc = self._l.pas_tas_gas_topk_policies_wide_after_device(
            self._h, tas_gen, gas_gen, n_pods, _dptr(pod_policy_t), _dptr(cand_t),
            max_containers, i915_index, _dptr(req_t), _dptr(mask_t), _dptr(ncont_t), k,
            node_base, _dptr(after_key_t), _dptr(after_sub_t), _dptr(after_node_t),
            _dptr(key_t), _dptr(sub_t), _dptr(node_t), _dptr(len_t), _stream(stream))
        self._check(rc, "pas_tas_gas_topk_policies_wide_after_device")
