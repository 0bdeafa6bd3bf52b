"""The byte-span arguments of every string verb answer alike (csrc/span_pool.hip:
check_host_spans, check_device_spans).

A batch of strings is "offsets [n + 1], bytes" (ByteSpans, csrc/csr_entry.h).  Every host form
refuses offsets that do not start at 0, offsets that decrease, and a null bytes pointer with a
non-zero total; every _device form refuses a negative byte count and a null bytes pointer with a
positive count.  Each is PAS_EINVAL and changes nothing: not the snapshots' generations or
content, not the name table, not the card-name table.

Shapes: a GAS snapshot of 4 nodes x 2 cards x 2 resources with its card-name table and a name
table, a TAS snapshot of 4 nodes x 2 metrics.  Every span argument under test holds two entries;
the other arguments of the call are valid, so the span is the only thing to refuse.  The calls go
through pas_amd._lib directly: the wrappers cannot pass a null bytes pointer."""
from ctypes import byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib

pytestmark = pytest.mark.gpu

N, K, Q, M = 4, 2, 2, 2
TAS_GEN, GAS_GEN = 11, 21
NODE_NAMES = [b"node-0", b"node-1", b"node-2", b"node-3"]
CARD_NAMES = [b"card0", b"card1"] * N


def pack(names):
    off = np.zeros(len(names) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in names])
    return off, np.frombuffer(b"".join(names) or b"\0", np.uint8).copy()


def ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


class Host:
    """Valid host spans of `names`, or the bad variant `case` of them."""
    CASES = ("from_1", "decrease", "negative", "null_bytes")

    def __init__(self, names, case=None):
        self.off, self.bytes = pack(names)
        assert len(names) == 2 or case is None
        if case == "from_1":
            self.off = np.array([1, 2, 3], np.int64)
        elif case == "decrease":
            self.off = np.array([0, 3, 2], np.int64)
        elif case == "negative":
            self.off = np.array([0, -1, 0], np.int64)
        elif case == "null_bytes":
            assert self.off[-1] > 0
            self.bytes = None

    def args(self):
        return (ptr(self.off), ptr(self.bytes))


class Device:
    """Valid device spans of `names`, or the bad variant `case` of them."""
    CASES = ("n_bytes_minus_1", "null_bytes")

    def __init__(self, names, case=None):
        import torch
        off, raw = pack(names)
        self.n_bytes = int(off[-1])
        self.off = torch.from_numpy(off).cuda()
        self.bytes = torch.from_numpy(raw).cuda()
        self.case = case

    def args(self):
        if self.case == "n_bytes_minus_1":
            return (-1, c_void_p(self.off.data_ptr()), c_void_p(self.bytes.data_ptr()))
        if self.case == "null_bytes":
            return (1, c_void_p(self.off.data_ptr()), None)
        return (self.n_bytes, c_void_p(self.off.data_ptr()), c_void_p(self.bytes.data_ptr()))


class World:
    """One context with every resident structure the verbs touch, and what they held at first."""

    def __init__(self):
        self.ctx = pas_amd.Context(0)
        self.reset()
        self.first = self.state()

    def reset(self):
        c = self.ctx
        rng = np.random.default_rng(5)
        vals = rng.integers(0, 1000, size=(M, N)).astype(np.int64)
        present = np.full((M, 1), (1 << N) - 1, np.uint64)
        c.tas_snapshot_set(TAS_GEN, vals, present)
        n_cards = np.full(N, K, np.int32)
        cap = np.full((N, Q), 1000, np.int64)
        used = rng.integers(0, 100, size=(N, K, Q)).astype(np.int64)
        c.gas_snapshot_set(GAS_GEN, n_cards, cap, used)
        off, raw = pack(NODE_NAMES)
        c.names_set(off, raw.tobytes())
        off, raw = pack(CARD_NAMES)
        c.gas_card_names_set(N, K, off, raw.tobytes())

    def state(self):
        c = self.ctx
        tas = c.tas_snapshot_get()
        gas = c.gas_snapshot_get()
        nodes = c.gas_snapshot_get_nodes()
        names = c.names_get()
        cards = c.gas_card_names_get()
        flat = []
        for part in (tas, gas, nodes, names, cards, c.names_info(), c.gas_card_names_info()):
            for x in part:
                flat.append(x.tobytes() if isinstance(x, np.ndarray) else x)
        return flat


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.ctx.close()


# ------------------------------------------------------------------ the forms
# form name -> (call, span arguments, has a _device twin).  call(w, S, spans) runs the form with
# spans[arg] an S (Host or Device) per span argument and returns the status.

def np32(*v):
    return np.array(v, np.int32)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def dp(t):
    return c_void_p(t.data_ptr())


LITS = [b"100m", b"2"]
ANNS = [b"card0", b"card1"]
LABELS = [b"card0.card1", b"card1"]


def pods():
    """Two pods of one container each"""
    return (np.ones((2, 1, Q), np.int64), np.full((2, 1), (1 << Q) - 1, np.uint32), np32(1, 1))


def quantities(w, S, sp):
    out = [np.zeros(2, t) for t in (np.int64, np.uint32, np.int32, np.int32)]
    if S is Host:
        return w.ctx._l.pas_quantities_to_wide(w.ctx._h, 2, *sp["lit"].args(), *map(ptr, out))
    outs = [dev(o) for o in out]
    return w.ctx._l.pas_quantities_to_wide_device(w.ctx._h, 2, *sp["lit"].args(), *map(dp, outs),
                                                  None)


def update_quantities(w, S, sp, by_name=False):
    l, h = w.ctx._l, w.ctx._h
    cols, col_off = np32(0), np.array([0, 2], np.int64)
    kind, scale, bad, unknown = np32(0), np32(0), c_int64(), c_int64()
    head = (h, TAS_GEN, TAS_GEN + 1, 1, ptr(cols), ptr(col_off))
    tail = (ptr(kind), ptr(scale), byref(bad))
    if by_name:
        fn = (l.pas_tas_snapshot_update_quantities_names if S is Host
              else l.pas_tas_snapshot_update_quantities_names_device)
        return fn(*head, *sp["name"].args(), *sp["lit"].args(), *tail, byref(unknown),
                  *(() if S is Host else (None,)))
    node = np32(0, 1)
    if S is Host:
        return l.pas_tas_snapshot_update_quantities(*head, ptr(node), *sp["lit"].args(), *tail)
    n_bytes, off, raw = sp["lit"].args()
    node_t = dev(node)
    return l.pas_tas_snapshot_update_quantities_device(*head, n_bytes, dp(node_t), off, raw, *tail,
                                                       None)


def names_set(w, S, sp):
    return w.ctx._l.pas_names_set(w.ctx._h, 2, *sp["name"].args())


def names_resolve(w, S, sp):
    slot = np32(0, 0)
    if S is Host:
        return w.ctx._l.pas_names_resolve(w.ctx._h, 2, *sp["name"].args(), ptr(slot))
    slot_t = dev(slot)
    return w.ctx._l.pas_names_resolve_device(w.ctx._h, 2, *sp["name"].args(), dp(slot_t), None)


def names_assign(w, S, sp):
    slot, new_entry, new_slot, n_new = np32(0, 0), np32(0, 0), np32(0, 0), c_int64()
    tail = (2, ptr(new_entry), ptr(new_slot), byref(n_new))
    if S is Host:
        return w.ctx._l.pas_names_assign(w.ctx._h, 2, *sp["name"].args(), ptr(slot), *tail)
    slot_t = dev(slot)
    return w.ctx._l.pas_names_assign_device(w.ctx._h, 2, *sp["name"].args(), dp(slot_t), *tail,
                                            None)


def card_names_set(w, S, sp):
    return w.ctx._l.pas_gas_card_names_set(w.ctx._h, 1, 2, *sp["name"].args())


def card_names_update(w, S, sp):
    return w.ctx._l.pas_gas_card_names_update(w.ctx._h, 1, ptr(np32(0)), *sp["name"].args())


def annotations_resolve(w, S, sp):
    pod, node, ncont = np32(0, 1), np32(0, 1), np32(1, 1)
    outs = [np.zeros(2, np.int32) for _ in range(4)]
    if S is Host:
        return w.ctx._l.pas_gas_annotations_resolve(
            w.ctx._h, 2, ptr(pod), ptr(node), 2, ptr(ncont), 1, *sp["ann"].args(), 1,
            *map(ptr, outs))
    keep = [dev(x) for x in (pod, node, ncont, *outs)]
    return w.ctx._l.pas_gas_annotations_resolve_device(
        w.ctx._h, 2, dp(keep[0]), dp(keep[1]), 2, dp(keep[2]), 1, *sp["ann"].args(), 1,
        *map(dp, keep[3:]), None)


def apply_annotations(w, S, sp, by_name=False):
    l, h = w.ctx._l, w.ctx._h
    kind, pod, node, st = np32(0, 0), np32(0, 1), np32(0, 1), np32(0, 0)
    req, mask, ncont = pods()
    if S is Host:
        conv, tail = ptr, ()
    else:
        keep = [dev(x) for x in (kind, pod, node, st, req, mask, ncont)]
        kind, pod, node, st, req, mask, ncont = keep
        conv, tail = dp, (None,)
    where = sp["name"].args() if by_name else (conv(node),)
    fn = getattr(l, "pas_gas_apply_annotations" + ("_names" if by_name else "") +
                 ("" if S is Host else "_device"))
    return fn(h, GAS_GEN, GAS_GEN + 1, 2, conv(kind), conv(pod), *where, 2, 1, conv(req),
              conv(mask), conv(ncont), *sp["ann"].args(), conv(st), *tail)


def node_strings(w, S, sp, by_name=False, update=True):
    l, h = w.ctx._l, w.ctx._h
    u = len(sp["label"].off) - 1
    node, state = np32(*range(u)), np.ones(u, np.int32)
    st, n_cards, gpus, dropped = (np.zeros(u, np.int32) for _ in range(4))
    cap, src, need = np.zeros(u * Q, np.int64), np.zeros(u * K, np.int32), c_int32()
    if S is Host:
        conv, tail = ptr, ()
    else:
        keep = [dev(x) for x in (node, state, st, n_cards, gpus, dropped, cap, src)]
        node, state, st, n_cards, gpus, dropped, cap, src = keep
        conv, tail = dp, (None,)
    where = sp["name"].args() if by_name else (conv(node),)
    strings = (*where, conv(state), *sp["label"].args(), *sp["lit"].args())
    sfx = "" if S is Host else "_device"
    if not update:
        return getattr(l, "pas_gas_nodes_resolve_strings" + sfx)(
            h, u, *strings, conv(st), conv(n_cards), conv(gpus), conv(cap), conv(src),
            conv(dropped), *tail)
    fn = getattr(l, "pas_gas_nodes_update_strings" + ("_names" if by_name else "") + sfx)
    return fn(h, GAS_GEN, GAS_GEN + 1, u, *strings, conv(st), conv(n_cards), conv(cap),
              conv(dropped), byref(need), *tail)


def named(f, **kw):
    return lambda w, S, sp: f(w, S, sp, **kw)


# (form, its span arguments with the two entries each holds in a valid call, has a _device twin)
FORMS = {
    "quantities_to_wide": (quantities, {"lit": LITS}, True),
    "tas_snapshot_update_quantities": (update_quantities, {"lit": LITS}, True),
    "tas_snapshot_update_quantities_names":
        (named(update_quantities, by_name=True), {"name": NODE_NAMES[:2], "lit": LITS}, True),
    "names_set": (names_set, {"name": NODE_NAMES[:2]}, False),
    "names_resolve": (names_resolve, {"name": NODE_NAMES[:2]}, True),
    "names_assign": (names_assign, {"name": NODE_NAMES[:2]}, True),
    "gas_card_names_set": (card_names_set, {"name": CARD_NAMES[:2]}, False),
    "gas_card_names_update": (card_names_update, {"name": CARD_NAMES[:2]}, False),
    "gas_annotations_resolve": (annotations_resolve, {"ann": ANNS}, True),
    "gas_apply_annotations": (apply_annotations, {"ann": ANNS}, True),
    "gas_apply_annotations_names":
        (named(apply_annotations, by_name=True), {"name": NODE_NAMES[:2], "ann": ANNS}, True),
    "gas_nodes_update_strings": (node_strings, {"label": LABELS, "lit": LITS}, True),
    "gas_nodes_update_strings_names":
        (named(node_strings, by_name=True),
         {"name": NODE_NAMES[:2], "label": LABELS, "lit": LITS}, True),
    "gas_nodes_resolve_strings":
        (named(node_strings, update=False), {"label": LABELS, "lit": LITS}, True),
}


def spans_for(S, form, bad_arg, case):
    """The form's span arguments, `bad_arg` in its bad variant.  The literals of a node update
    come Q = 2 per update: with them under test the batch is one update, else two."""
    _, args, _ = FORMS[form]
    node_form = "label" in args
    u = 1 if node_form and bad_arg == "lit" else 2
    out = {}
    for arg, names in args.items():
        if node_form:
            names = (names * Q)[:u * Q] if arg == "lit" else names[:u]
        out[arg] = S(names, case if arg == bad_arg else None)
    return out


def cases(S, device):
    return [pytest.param(form, arg, case, id=f"{form}-{arg}-{case}")
            for form, (_, args, twin) in FORMS.items() if twin or not device
            for arg in args for case in S.CASES]


def refused(w, S, form, arg, case):
    rc = FORMS[form][0](w, S, spans_for(S, form, arg, case))
    assert rc == _lib.PAS_EINVAL, (rc, w.ctx.last_error())
    msg = w.ctx.last_error()
    assert msg.startswith("pas_" + form), msg
    assert any(x in msg for x in ("offsets", "bytes", "byte count")), msg  # the span check's
    assert w.state() == w.first, "a refused call changed resident state"


@pytest.mark.parametrize("form,arg,case", cases(Host, False))
def test_host_form_refuses_bad_spans(world, form, arg, case):
    refused(world, Host, form, arg, case)


@pytest.mark.parametrize("form,arg,case", cases(Device, True))
def test_device_form_refuses_bad_spans(world, form, arg, case):
    refused(world, Device, form, arg, case)


@pytest.mark.parametrize("form", list(FORMS))
def test_valid_spans_pass(form):
    """The same calls with nothing wrong succeed, host form and _device twin, each on a context
    of its own set up afresh (most forms write), so the refusals above are the spans' doing."""
    w = World()
    try:
        for S in (Host, Device) if FORMS[form][2] else (Host,):
            w.reset()
            rc = FORMS[form][0](w, S, spans_for(S, form, None, None))
            assert rc == _lib.PAS_OK, (S.__name__, w.ctx.last_error())
            w.ctx.synchronize()
    finally:
        w.ctx.close()
