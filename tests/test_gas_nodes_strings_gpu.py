"""Node events from strings on the device (csrc/gas_node_strings.hip) against the route the cache
takes today, run on a second context: snapshot.gas_node_row + snapshot.card_remap +
pas_gas_nodes_update + pas_gas_card_names_update, with pas_quantity_as_int64 for the literals.
Every comparison is exact: statuses, counts, capacities, the resident usage and the names.

Shapes: N = 65 node slots, Q = 3 resource kinds, max_cards k in {8, 16, 64}."""
import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd.snapshot import (GPU_LIST_LABEL, card_remap, gas_node_row, pack_card_names,
                              pack_names, pack_node_strings)

N, Q = 65, 3
KINDS = ["gpu.intel.com/i915", "gpu.intel.com/memory.max", "gpu.intel.com/millicores"]
TIERS = [8, 16, 64]
OK, ERR = _lib.PAS_GAS_OK, _lib.PAS_GAS_ERR_INPUT
LONG = "L" * 70  # names past 64 bytes that differ in the last byte
ODD = ["", "a\x00b", "a\x00a", "é", "ÿ", "z\U0001f600", LONG + "a", LONG + "b", "card1",
       "card10", "card2"]


def node(cards, alloc=("8", "8000", "800")):
    """A node dict as gas_node_row reads it: cards None = no label; alloc entries None = a kind
    the node does not advertise."""
    labels = {} if cards is None else {GPU_LIST_LABEL: ".".join(cards)}
    return {"labels": labels,
            "allocatable": {k: v for k, v in zip(KINDS, alloc) if v is not None}}


def names(k, count, salt=0):
    """`count` distinct card names, the odd ones first."""
    pool = ODD + [f"gpu{salt}-{i}" for i in range(k + 2)]
    return pool[:count]


class Capacity(Exception):
    pass


class Ref:
    """The host route on its own context, one update per call."""

    def __init__(self, ctx, k, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.k, self.gen = ctx, k, 7
        self.rows, self.n_cards = [], np.zeros(N, np.int32)
        used = np.zeros((N, k, Q), np.int64)
        for s in range(N):
            label = sorted(names(k, s % (k + 1), salt=s % 3), key=lambda c: c.encode())
            self.n_cards[s] = len(label)
            self.rows.append(label + [""] * (k - len(label)))
            used[s, :len(label)] = rng.integers(1, 1 << 40, (len(label), Q))
        self.cap = rng.integers(0, 1 << 30, (N, Q)).astype(np.int64)
        self.used0 = used

    def install(self, ctx):
        ctx.gas_snapshot_set(self.gen, self.n_cards, self.cap, self.used0)
        ctx.gas_card_names_set(N, self.k, *pack_card_names(self.rows, None, self.k))
        ctx.names_set(*pack_names([f"node-{s}" for s in range(N)]))

    def plan(self, slot, nd):
        """(n_cards, cap, gpu_count, src, new_row or None, dropped) of one update."""
        k, row = self.k, self.rows[slot]
        n_old = max(int(self.n_cards[slot]), 0)
        n_cards, cap, cards = gas_node_row(nd, KINDS)
        if nd is None or GPU_LIST_LABEL not in nd["labels"]:
            return n_cards, cap, 0, list(range(k)), None, 0
        if len(cards) > k:
            raise Capacity(len(cards))
        live = [(j, c) for j, c in enumerate(row) if not (c == "" and j >= n_old)]
        src_c, new_slots, dropped = card_remap([c for _, c in live], cards, k)
        src = [live[s][0] if s >= 0 else -1 for s in src_c]
        for i, c in enumerate(new_slots[:n_cards]):
            if src[i] < 0 and c == "" and "" in row:  # an unused slot: zero usage either way
                src[i] = row.index("")
        return (n_cards, cap, len(nd["labels"][GPU_LIST_LABEL].split(".")), src,
                new_slots + [""] * (k - len(new_slots)), len(dropped))

    def apply(self, slot, nd):
        n_cards, cap, _, src, new_row, dropped = self.plan(slot, nd)
        st = self.ctx.gas_nodes_update(self.gen, self.gen + 1, [slot], [n_cards], [cap], [src])
        assert list(st) == [OK]
        self.gen += 1
        if new_row is not None:
            self.ctx.gas_card_names_update([slot], *pack_card_names([new_row], None, self.k))
            self.rows[slot] = new_row
        self.n_cards[slot] = n_cards
        return n_cards, cap, dropped


def table_rows(ctx):
    n, k, _ = ctx.gas_card_names_info()
    off, blob = ctx.gas_card_names_get()
    flat = [blob[off[i]:off[i + 1]] for i in range(n * k)]
    return [flat[s * k:(s + 1) * k] for s in range(n)]


def state(ctx):
    _, used = ctx.gas_snapshot_get()
    _, n_cards, cap = ctx.gas_snapshot_get_nodes()
    return used, n_cards, cap, table_rows(ctx)


def assert_same_state(ctx, ref):
    got, want = state(ctx), state(ref.ctx)
    assert np.array_equal(got[0], want[0]), "usage"
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), "n_cards / cap"
    assert got[3] == want[3], "card names"
    assert want[3] == [[c.encode() for c in row] for row in ref.rows]


@pytest.fixture(scope="module")
def ref_ctx():
    c = pas_amd.Context(0)
    yield c
    c.close()


class Pair:
    def __init__(self, ctx, ref_ctx, k, seed=1):
        self.ctx, self.ref, self.gen = ctx, Ref(ref_ctx, k, seed), 7
        self.ref.install(ctx)
        self.ref.install(ref_ctx)

    def send(self, slots, nodes, by_name=False):
        """One strings call on the device route, update by update on the host route; the
        outputs compared update by update, then the resident state."""
        packed = pack_node_strings(nodes, KINDS)
        if by_name:
            out = self.ctx.gas_nodes_update_strings_names(
                self.gen, self.gen + 1, *pack_names([f"node-{s}" for s in slots]), *packed)
        else:
            out = self.ctx.gas_nodes_update_strings(self.gen, self.gen + 1, slots, *packed)
        self.gen += 1
        st, n_cards, cap, dropped = out
        for u, (slot, nd) in enumerate(zip(slots, nodes)):
            want = self.ref.apply(slot, nd)
            assert st[u] == OK
            assert (n_cards[u], list(cap[u]), dropped[u]) == (want[0], list(want[1]), want[2]), u
        assert_same_state(self.ctx, self.ref)
        return out


def mixed_batch(k, u_count, seed):
    """u_count updates over the 65 slots (a slot repeats once u_count passes 65): every kind of
    label and literal the grammar has."""
    rng = np.random.default_rng(seed)
    allocs = [("8", "8000", "800"), ("-7", "1e19", "9e18"), ("1.5", None, "16Ki"),
              (None, None, None), ("9223372036854775807", "-9e18", "1000m"), ("12k", "007", "+5")]
    slots, nodes = [], []
    for u in range(u_count):
        slot = (u * 7) % N
        kind = u % 9
        if kind == 0:
            nd = None                                             # gone
        elif kind == 1:
            nd = node(None)                                       # no label
        elif kind == 2:
            nd = node(names(k, k, salt=u % 3))                    # exactly k distinct cards
        elif kind == 3:
            cards = names(k, max(1, k // 2), salt=1)
            nd = node(cards + cards[:2] + cards[:1])              # duplicates: gpuCount > n_cards
        elif kind == 4:
            nd = node(["card2", "card10", "card1", ""])           # sort.Strings order, "" first
        elif kind == 5:
            nd = node([LONG + "b", LONG + "a", "a\x00b", "a\x00a", "é", "ÿ"])
        elif kind == 6:
            nd = node([""])                                       # the empty label: one card ""
        else:
            take = rng.permutation(k + 2)[:int(rng.integers(1, k + 1))]
            nd = node([names(k, k + 2, salt=u % 3)[i] for i in take])
        if nd is not None:
            nd["allocatable"] = {kk: v for kk, v in zip(KINDS, allocs[u % len(allocs)])
                                 if v is not None}
        slots.append(slot)
        nodes.append(nd)
    return slots, nodes


@pytest.mark.gpu
@pytest.mark.parametrize("k", TIERS)
@pytest.mark.parametrize("u_count", [1, 63, 64, 65, 257])
def test_batches_match_the_host_route(ctx, ref_ctx, k, u_count):
    """U in {1, 63, 64, 65, 257}; 257 updates over 65 slots is every node four times in one
    call (four rounds)."""
    pair = Pair(ctx, ref_ctx, k, seed=u_count)
    slots, nodes = mixed_batch(k, u_count, seed=k + u_count)
    st, n_cards, cap, _ = pair.send(slots, nodes)
    if u_count >= 63:  # the batch reaches the division and its signs
        assert (cap < 0).any() and (n_cards == k).any() and (n_cards == -1).any()
    assert ctx.gas_snapshot_info()[0] == pair.gen


@pytest.mark.gpu
@pytest.mark.parametrize("k", TIERS)
def test_one_node_two_and_three_times_in_one_call(ctx, ref_ctx, k):
    pair = Pair(ctx, ref_ctx, k)
    a, b, c = names(k, k + 2, salt=2)[-3:]
    pair.send([5, 9, 5], [node([a, b]), node([c]), node([b, c])])
    pair.send([5, 5, 5, 9], [node([a]), None, node([a, b, c]), node(None)])


@pytest.mark.gpu
@pytest.mark.parametrize("k", TIERS)
def test_cards_leave_are_parked_return_and_are_dropped(ctx, ref_ctx, k):
    pair = Pair(ctx, ref_ctx, k)
    slot = k  # the slot whose initial label fills the row
    full = [c for c in pair.ref.rows[slot]]
    assert len(set(full)) == k and pair.ref.n_cards[slot] == k
    keep = [c for c in full if c != ""]
    out = pair.send([slot], [node(keep[:2])])               # k - 2 cards leave: all parked
    assert out[3][0] == 0 and pair.ref.rows[slot].count("") == 1
    fresh = [f"new{i}" for i in range(3)]
    out = pair.send([slot], [node(keep[:2] + fresh)])       # the row is full: parked cards drop
    assert out[3][0] == 2                                   # ("" outside the label is no card)
    home = ctx.gas_snapshot_get()[1][slot][pair.ref.rows[slot].index(keep[2])].copy()
    assert home.all()
    pair.send([slot], [node(keep[:4])])                     # parked cards return with their usage
    assert pair.ref.rows[slot].index(keep[2]) < 4
    assert np.array_equal(ctx.gas_snapshot_get()[1][slot][pair.ref.rows[slot].index(keep[2])],
                          home)
    pair.send([slot], [None])                                # gone: the row stays
    assert ctx.gas_snapshot_get_nodes()[1][slot] == -1
    pair.send([slot], [node(keep[:3])])                      # ... and has its usage when it returns
    pair.send([slot], [node(None)])
    pair.send([slot], [node(keep[1:5])])


@pytest.mark.gpu
@pytest.mark.parametrize("k", TIERS)
def test_capacity_reports_need_cards_and_changes_nothing(ctx, ref_ctx, k):
    pair = Pair(ctx, ref_ctx, k)
    before = state(ctx)
    big = [f"c{i:03d}" for i in range(k + 1)]
    with pytest.raises(_lib.PasError) as e:
        ctx.gas_nodes_update_strings(pair.gen, pair.gen + 1, [3, 4],
                                     *pack_node_strings([node(["a"]), node(big)], KINDS))
    assert e.value.code == _lib.PAS_ECAPACITY and e.value.need_cards == k + 1
    if k == 64:  # the count stops at PAS_GAS_MAX_CARDS + 1
        with pytest.raises(_lib.PasError) as e:
            ctx.gas_nodes_update_strings(pair.gen, pair.gen + 1, [4], *pack_node_strings(
                [node([f"c{i}" for i in range(200)])], KINDS))
        assert e.value.need_cards == 65
    after = state(ctx)
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3]))
    assert before[3] == after[3] and ctx.gas_snapshot_info()[0] == pair.gen
    pair.send([4], [node(big[:k])])  # exactly k fits, at the same generation


@pytest.mark.gpu
def test_bad_literal_is_err_input_and_leaves_the_row(ctx, ref_ctx):
    pair = Pair(ctx, ref_ctx, 8)
    before = state(ctx)
    nodes = [node(["x", "y"], ("4", "4x", "1")), node(["x"], ("1", "2", "3")),
             node(["q"], ("1\x002", "2", "3")), node(["q"], ("", None, "1K"))]
    st, n_cards, cap, dropped = ctx.gas_nodes_update_strings(
        pair.gen, pair.gen + 1, [1, 2, 3, 4], *pack_node_strings(nodes, KINDS))
    pair.gen += 1
    assert list(st) == [ERR, OK, ERR, ERR]
    assert list(n_cards) == [0, 1, 0, 0] and not cap[[0, 2, 3]].any() and list(cap[1]) == [1, 2, 3]
    pair.ref.apply(2, nodes[1])
    assert_same_state(ctx, pair.ref)
    assert before[3][1] == table_rows(ctx)[1]


@pytest.mark.gpu
def test_names_form(ctx, ref_ctx):
    pair = Pair(ctx, ref_ctx, 16)
    pair.send([3, 64, 0], [node(["b", "a"]), None, node(None)], by_name=True)
    nodes = [node(["a"]), None, node(["a"]), node(["z"]), node(["z"])]
    noff, nblob = pack_names(["", "ghost", "ghost", "node-7", "node-8"])
    states, *rest = pack_node_strings(nodes, KINDS)
    states[4] = 5  # a state outside {-1, 0, 1}
    with pytest.raises(_lib.PasError) as e:  # the host form checks the states
        ctx.gas_nodes_update_strings_names(pair.gen, pair.gen + 1, noff, nblob, states, *rest)
    assert e.value.code == _lib.PAS_EINVAL
    states[4] = _lib.PAS_GAS_NODE_LABEL
    st, n_cards, _, _ = ctx.gas_nodes_update_strings_names(pair.gen, pair.gen + 1, noff, nblob,
                                                           states, *rest)
    pair.gen += 1
    # an empty name; a name without a slot that is gone; the same with a label; two real ones
    assert list(st) == [ERR, OK, ERR, OK, OK] and list(n_cards) == [0, -1, 0, 1, 1]
    pair.ref.apply(7, nodes[3])
    pair.ref.apply(8, nodes[4])
    assert_same_state(ctx, pair.ref)


@pytest.mark.gpu
def test_generation_tables_and_shape_errors(ctx, ref_ctx):
    pair = Pair(ctx, ref_ctx, 8)
    packed = pack_node_strings([node(["a"])], KINDS)
    before = state(ctx)

    def code(fn, *a):
        with pytest.raises(_lib.PasError) as e:
            fn(*a)
        return e.value.code, str(e.value)

    assert code(ctx.gas_nodes_update_strings, pair.gen + 1, pair.gen + 2, [0],
                *packed)[0] == _lib.PAS_ESTALE
    assert code(ctx.gas_nodes_update_strings, pair.gen, pair.gen + 1, [N],
                *packed)[0] == _lib.PAS_EINVAL                      # a slot outside the snapshot
    bad_off = (packed[0], np.array([1, 1], np.int64)) + packed[2:]
    assert code(ctx.gas_nodes_update_strings, pair.gen, pair.gen + 1, [0],
                *bad_off)[0] == _lib.PAS_EINVAL                     # offsets must start at 0
    bad_off = packed[:3] + (np.array([0, 3, 2, 4], np.int64), packed[4])
    assert code(ctx.gas_nodes_update_strings, pair.gen, pair.gen + 1, [0],
                *bad_off)[0] == _lib.PAS_EINVAL                     # ... and never decrease
    ctx.names_drop()
    noff, nblob = pack_names(["node-1"])
    assert code(ctx.gas_nodes_update_strings_names, pair.gen, pair.gen + 1, noff, nblob,
                *packed)[0] == _lib.PAS_ENOSNAP
    ctx.gas_card_names_resize(N, 16)
    c, msg = code(ctx.gas_nodes_update_strings, pair.gen, pair.gen + 1, [0], *packed)
    assert c == _lib.PAS_EINVAL and "card-name table" in msg
    assert code(ctx.gas_nodes_resolve_strings, [0], *packed)[0] == _lib.PAS_EINVAL
    ctx.gas_card_names_drop()
    assert code(ctx.gas_nodes_update_strings, pair.gen, pair.gen + 1, [0],
                *packed)[0] == _lib.PAS_ENOSNAP
    assert code(ctx.gas_card_names_get_rows, [0])[0] == _lib.PAS_ENOSNAP
    after_used, after_n, after_cap = ctx.gas_snapshot_get()[1], *ctx.gas_snapshot_get_nodes()[1:]
    assert np.array_equal(before[0], after_used) and np.array_equal(before[1], after_n)
    assert np.array_equal(before[2], after_cap) and ctx.gas_snapshot_info()[0] == pair.gen


@pytest.mark.gpu
@pytest.mark.parametrize("k", TIERS)
def test_resolve_form_matches_the_host_route_and_writes_nothing(ctx, ref_ctx, k):
    pair = Pair(ctx, ref_ctx, k)
    slots, nodes = mixed_batch(k, 65, seed=3 * k)  # every slot once: all against the resident rows
    before = state(ctx)
    st, n_cards, gpus, cap, src, dropped = ctx.gas_nodes_resolve_strings(
        slots, *pack_node_strings(nodes, KINDS))
    assert list(st) == [OK] * 65
    for u, (slot, nd) in enumerate(zip(slots, nodes)):
        w_cards, w_cap, w_gpus, w_src, _, w_dropped = pair.ref.plan(slot, nd)
        assert (n_cards[u], gpus[u], dropped[u]) == (w_cards, w_gpus, w_dropped), u
        assert list(cap[u]) == list(w_cap) and list(src[u]) == w_src, u
    assert (gpus > n_cards).any()
    after = state(ctx)
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3]))
    assert before[3] == after[3] and ctx.gas_snapshot_info()[0] == pair.gen
    # a label past max_cards is reported, not resolved
    st, n_cards, _, _, src, _ = ctx.gas_nodes_resolve_strings(
        [0], *pack_node_strings([node([f"c{i}" for i in range(k + 1)])], KINDS))
    assert (st[0], n_cards[0]) == (OK, k + 1) and (src[0] == -1).all()


@pytest.mark.gpu
def test_device_form_reads_its_offsets_clamped(ctx, ref_ctx):
    import torch
    pair = Pair(ctx, ref_ctx, 8)
    dev = torch.device("cuda:0")
    label_blob, cap_blob = b"b.a.card7.x", b"8" + b"16" + b"4Ki"
    # offsets outside the blobs on both sides, and ends before their begins (empty spans)
    label_off = [-50, 3, 1, 4, 1 << 40]
    cap_off = [-9, 1, 3, 1 << 50, 2, 1, 0, 0, 0, 0, 0, 1, 1]
    clamp = lambda off, n: [min(max(o, 0), n) for o in off]
    lo, co = clamp(label_off, len(label_blob)), clamp(cap_off, len(cap_blob))
    span = lambda blob, off, i: blob[off[i]:max(off[i + 1], off[i])]
    want_nodes = []
    for u in range(4):
        lits = [span(cap_blob, co, u * Q + q).decode() or None for q in range(Q)]
        want_nodes.append(node(span(label_blob, lo, u).decode().split("."), lits))
    assert [n["labels"][GPU_LIST_LABEL] for n in want_nodes] == ["b.a", "", ".a.", "card7.x"]
    assert want_nodes[0]["allocatable"] == dict(zip(KINDS, ["8", "16", "4Ki"]))
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    status = torch.full((4,), -9, dtype=torch.int32, device=dev)
    n_cards = torch.full((4,), -9, dtype=torch.int32, device=dev)
    cap = torch.full((4, Q), -9, dtype=torch.int64, device=dev)
    args = (t([10, 11, 12, 13], torch.int32), t([1, 1, 1, 1], torch.int32), len(label_blob),
            t(label_off, torch.int64), t(list(label_blob), torch.uint8), len(cap_blob),
            t(cap_off, torch.int64), t(list(cap_blob), torch.uint8))
    torch.cuda.synchronize()
    need = ctx.gas_nodes_update_strings_device(pair.gen, pair.gen + 1, 4, *args, status, n_cards,
                                               cap)
    ctx.synchronize()
    torch.cuda.synchronize()
    pair.gen += 1
    assert need == 2 and status.tolist() == [OK] * 4
    for u, nd in enumerate(want_nodes):
        w_cards, w_cap, _ = pair.ref.apply(10 + u, nd)
        assert n_cards[u].item() == w_cards and cap[u].tolist() == list(w_cap)
    assert_same_state(ctx, pair.ref)


@pytest.mark.gpu
@pytest.mark.parametrize("k", TIERS)
def test_get_rows_against_get(ctx, ref_ctx, k):
    Pair(ctx, ref_ctx, k)
    rows = table_rows(ctx)
    pick = [64, 0, k, 7, 7, 33]
    assert ctx.gas_card_names_get_rows(pick) == [rows[s] for s in pick]
    assert ctx.gas_card_names_get_rows([]) == []
    with pytest.raises(_lib.PasError) as e:
        ctx.gas_card_names_get_rows([N])
    assert e.value.code == _lib.PAS_EINVAL
    # a buffer one byte short: PAS_ECAPACITY with the offsets delivered
    want = sum(map(len, rows[k]))
    off = np.zeros(k + 1, np.int64)
    buf = np.zeros(want, np.uint8)
    slot = np.array([k], np.int32)
    rc = ctx._l.pas_gas_card_names_get_rows(ctx._h, 1, slot.ctypes.data, off.ctypes.data,
                                            buf.ctypes.data, want - 1)
    assert rc == _lib.PAS_ECAPACITY and off[-1] == want


@pytest.mark.gpu
def test_one_row_rewritten_until_the_pool_gathers(ctx, ref_ctx):
    pair = Pair(ctx, ref_ctx, 8)
    sizes = [ctx.gas_card_names_info()[2]]
    for i in range(40):  # a long name per rewrite: the dead bytes pass the live ones
        pair.send([9], [node([f"{'n' * 200}{i}", "stay"])])
        assert ctx.gas_card_names_info() == pair.ref.ctx.gas_card_names_info()
        sizes.append(ctx.gas_card_names_info()[2])
    assert any(b < a for a, b in zip(sizes, sizes[1:])), "the pool never gathered"
