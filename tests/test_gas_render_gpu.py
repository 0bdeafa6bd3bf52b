"""Bind annotations and node names rendered on the device (pas_gas_annotations_render[_ranks],
pas_names_render and their _device forms, csrc/gas_render.hip; place_to_completion(annotate=True);
GASExtender(device_annotations=True)).

The reference answer is snapshot.annotation_counts, the host restatement of bindNode
(scheduler.go:317-335) that the extender tests pin, with the status rules of include/pas.h
restated beside it.  The second reference is the resident parser: pas_gas_annotations_resolve of
the rendered bytes gives back the ranks and cards per container that went in.

Shapes: N = 65 node slots, k in {8, 16, 64}, C in {1, 3, 8} (C * k crosses several wavefronts at
8 x 64), B in {0, 1, 63, 64, 65, 257} (the 4-binds-per-block edge and several blocks).  Card names
have lengths from {0, 1, 5, 6, 63, 64, 65, 300} and hold byte 0 and bytes >= 0x80; counts come
from {0, 1, 2, 70, 1000}."""
import functools
import json

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd import workload as wl
from pas_amd.snapshot import annotation_counts, go_sort_strings, pack_names

OK, ERR_INPUT, ERR_OVERFLOW = _lib.PAS_GAS_OK, _lib.PAS_GAS_ERR_INPUT, _lib.PAS_GAS_ERR_OVERFLOW
N = 65
Q = 3
NAME_LENS = [0, 1, 5, 6, 63, 64, 65, 300]
COUNTS = [0, 1, 2, 70, 1000]
NODE_NAMES = [f"node-{n}" for n in range(N)]
SHAPES = [(8, 1), (8, 3), (16, 3), (64, 3), (64, 8), (16, 8)]
BS = [0, 1, 63, 64, 65, 257]


# ------------------------------------------------------------------ inputs and reference

def card_rows(rng, n_cards, k):
    """Rows of k distinct names without ',' and '|': name c of a row starts with a byte of its
    own (so no two are equal) and has a length from NAME_LENS; one name of a row is empty."""
    alphabet = np.array([b for b in range(256) if b not in (ord(","), ord("|"))], np.uint8)
    rows = []
    for n in range(len(n_cards)):
        lens = rng.choice(NAME_LENS[1:], size=k, p=[.2, .3, .3, .05, .05, .05, .05])
        lens[rng.integers(0, k)] = 0
        row = []
        for c in range(k):
            body = rng.choice(alphabet, size=int(lens[c]))
            if lens[c]:
                body[0] = alphabet[c]  # k <= 64 < len(alphabet)
            row.append(body.tobytes())
        rows.append(row)
    return rows


def ref_render(node, nc, counts, n_cards, rows, k):
    """(status, bytes) of one bind by the rules of include/pas.h."""
    if node == -1:
        return OK, b""
    if node < 0 or node >= len(rows):
        return ERR_INPUT, b""
    L = max(0, min(int(n_cards[node]), k))
    c = counts[:nc]
    if (c < 0).any() or (c[:, L:] != 0).any():
        return ERR_INPUT, b""
    length = sum(int(c[s, j]) * (len(rows[node][j]) + 1) for s in range(nc) for j in range(L))
    if length > 2**33:  # (far past the limit: no string is built)
        return ERR_OVERFLOW, b""
    names = [r.decode("latin-1") for r in rows[node][:L]]
    out = annotation_counts(c[:, :L], nc, names).encode("latin-1")
    return (ERR_OVERFLOW, b"") if len(out) > 2**31 - 1 else (OK, out)


@functools.lru_cache(maxsize=None)
def table_case(k):
    rng = np.random.default_rng(4200 + k)
    n_cards = rng.integers(1, k + 1, size=N).astype(np.int32)
    n_cards[0] = k          # a full row
    n_cards[1] = k // 2     # a parked card stands behind the label cards
    n_cards[2] = 0          # no cards label
    n_cards[3] = -1         # a node the lister does not know
    rows = card_rows(rng, n_cards, k)
    n_cards.setflags(write=False)
    return n_cards, rows


@functools.lru_cache(maxsize=None)
def bind_case(k, C, B):
    """B binds over table_case(k), with their reference statuses and bytes, the ranks form of the
    same binds, and the indices of the binds that are errors by construction."""
    n_cards, rows = table_case(k)
    rng = np.random.default_rng(1000 * k + 10 * C + B)
    node = rng.integers(0, N, size=B).astype(np.int32)
    ncont = rng.integers(0, C + 1, size=B).astype(np.int32)
    counts = np.zeros((B, C, k), np.int64)
    for b in range(B):
        L = max(int(n_cards[node[b]]), 0)
        for c in range(int(ncont[b])):
            for j in rng.integers(0, max(L, 1), size=int(rng.integers(0, 4))):
                if L:
                    counts[b, c, j] = rng.choice(COUNTS, p=[.1, .6, .2, .07, .03])
            if L and b % 16 == 9:   # many cards of one container
                counts[b, c, :L] = rng.integers(0, 3, size=L)
            lone = counts[b, c].sum() == 1 and len(rows[node[b]][int(counts[b, c].argmax())]) == 0
            if lone:  # (the empty name alone is the empty segment: not a round trip)
                counts[b, c] *= 2
    special = {}
    if B >= 63:
        node[5] = node[20] = -1                      # unplaced pods
        counts[5] = counts[20] = 0
        special = {"negative": 11, "parked": 30, "overflow": 41, "no label": 50}
        node[11], ncont[11] = 0, C
        counts[11, C - 1, k - 1] = -1
        node[30], ncont[30] = 1, C
        counts[30, 0, k // 2] = 1                    # the parked slot of row 1
        node[41], ncont[41] = 0, C
        counts[41, 0, 3] = 2**62
        node[50], ncont[50] = 2, max(C, 1)
        counts[50, 0, 0] = 1                         # n_cards 0: no slot may be selected
        named = next(j for j in range(k) if rows[0][j])
        for b in special.values():                   # good binds that render bytes around each
            for nb in (b - 1, b + 1):
                node[nb], ncont[nb], counts[nb] = 0, C, 0
                counts[nb, C - 1, named] = 2
    want = [ref_render(int(node[b]), int(ncont[b]), counts[b], n_cards, rows, k) for b in range(B)]
    status = np.array([w[0] for w in want], np.int32).reshape(B)
    off = np.zeros(B + 1, np.int64)
    np.cumsum([len(w[1]) for w in want], out=off[1:])
    # the ranks form: the containers' cards consecutively (the huge counts stay out of it)
    listed = [[[j for j in range(k) for _ in range(int(min(counts[b, c, j], 1000)))]
               for c in range(int(ncont[b]))] for b in range(B)]
    for b in special.values():
        listed[b] = [[] for _ in range(int(ncont[b]))]
    ld = max([1] + [sum(len(s) for s in row) for row in listed])
    cpc = np.zeros((B, C), np.int32)
    cards = np.full((B, ld), -1, np.int32)
    for b, row in enumerate(listed):
        flat = [j for s in row for j in s]
        cpc[b, :len(row)] = [len(s) for s in row]
        cards[b, :len(flat)] = flat
    case = dict(node=node, ncont=ncont, counts=counts, status=status, off=off, cpc=cpc,
                cards=cards)
    for a in case.values():
        a.setflags(write=False)
    case.update(blob=b"".join(w[1] for w in want), special=special, k=k, C=C, B=B, ld=ld)
    return case


def ranks_expectation(i):
    """The ranks form renders what the counts form does, except the binds built as errors of the
    counts form, which list nothing."""
    n_cards, rows = table_case(i["k"])
    want = []
    for b in range(i["B"]):
        counts = np.zeros((i["C"], i["k"]), np.int64)
        pos = 0
        for c in range(i["C"]):
            for j in i["cards"][b, pos:pos + i["cpc"][b, c]]:
                counts[c, j] += 1
            pos += i["cpc"][b, c]
        want.append(ref_render(int(i["node"][b]), int(i["ncont"][b]), counts, n_cards, rows,
                               i["k"]))
    return want


# ------------------------------------------------------------------ CPU: the cases' own reach

def test_cases_reach_what_they_claim():
    residues, lens_seen, counts_seen = set(), set(), set()
    for k, C in SHAPES:
        n_cards, rows = table_case(k)
        lens_seen |= {len(c) for row in rows for c in row}
        assert any(b"\x00" in c for row in rows for c in row)
        assert any(max(c, default=0) >= 0x80 for row in rows for c in row)
        assert all(len(set(row)) == k for row in rows)
        i = bind_case(k, C, 257)
        counts_seen |= set(np.unique(i["counts"][i["status"] == OK]).tolist())
        residues |= set((i["off"][:-1] % 16).tolist())
        for what, b in i["special"].items():
            assert i["status"][b] == (ERR_OVERFLOW if what == "overflow" else ERR_INPUT), what
            assert i["status"][b - 1] == OK and i["status"][b + 1] == OK
            assert i["off"][b] < i["off"][b + 2]  # a neighbour renders bytes
        assert (i["node"] == -1).sum() >= 2 and (i["status"] == OK).sum() >= 240
        assert i["off"][-1] < 8 << 20
        assert i["blob"].count(b"|") >= 1 or C == 1
    assert lens_seen == set(NAME_LENS) and set(COUNTS) <= counts_seen
    assert residues == set(range(16))  # bind starts on every byte residue


# ------------------------------------------------------------------ GPU plumbing

_gen = [93000]


def upload(ctx, k):
    n_cards, rows = table_case(k)
    _gen[0] += 10
    ctx.gas_snapshot_set(_gen[0], n_cards, np.zeros((N, Q), np.int64),
                         np.zeros((N, k, Q), np.int64))
    ctx.gas_card_names_set(N, k, *pack_blobs([c for row in rows for c in row]))
    return _gen[0]


def pack_blobs(names):
    off = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(n) for n in names], out=off[1:])
    return off, b"".join(names)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def render_device(ctx, i, form, cap=None, guard=64):
    """The _device form on tensors: (status, off, bytes with `guard` bytes of 0xAB behind cap,
    total or the PasError)."""
    import torch
    B, C = i["B"], i["C"]
    status = torch.full((max(B, 1),), -9, dtype=torch.int32, device="cuda")
    off = torch.full((B + 1,), -9, dtype=torch.int64, device="cuda")
    head = (B, dev(i["node"]), dev(i["ncont"]), C)
    if form == "counts":
        call, args = ctx.gas_annotations_render_device, head + (dev(i["counts"]),)
    else:
        call = ctx.gas_annotations_render_ranks_device
        args = head + (dev(i["cpc"]), dev(i["cards"]), i["ld"])
    if cap is None:
        try:
            cap = call(*args, status, off, None, 0)
        except _lib.PasError as e:
            assert e.code == _lib.PAS_ECAPACITY
            cap = e.n_bytes
    out = torch.full((cap + guard,), 0xAB, dtype=torch.uint8, device="cuda")
    try:
        total = call(*args, status, off, out, cap)
    except _lib.PasError as e:
        total = e
    torch.cuda.synchronize()
    return status[:B].cpu().numpy(), off.cpu().numpy(), out.cpu().numpy(), total


# ------------------------------------------------------------------ render parity

@pytest.mark.gpu
@pytest.mark.parametrize("k,C", SHAPES)
@pytest.mark.parametrize("B", BS)
def test_counts_form_matches_the_reference(ctx, k, C, B):
    i = bind_case(k, C, B)
    upload(ctx, k)
    status, off, out, total = render_device(ctx, i, "counts")
    assert total == i["off"][-1]
    np.testing.assert_array_equal(status, i["status"])
    np.testing.assert_array_equal(off, i["off"])
    assert out[:total].tobytes() == i["blob"]
    assert (out[total:] == 0xAB).all()
    for b in i["special"].values():  # an empty span between untouched neighbours
        assert off[b] == off[b + 1]
    # the host form is the device form
    st_h, anns = ctx.gas_annotations_render(i["node"], i["ncont"], i["counts"])
    np.testing.assert_array_equal(st_h, i["status"])
    assert anns == [i["blob"][i["off"][b]:i["off"][b + 1]] for b in range(B)]


@pytest.mark.gpu
@pytest.mark.parametrize("k,C", SHAPES)
@pytest.mark.parametrize("B", [0, 1, 65, 257])
def test_ranks_form_matches_the_reference_and_the_parser(ctx, k, C, B):
    import torch
    i = bind_case(k, C, B)
    want = ranks_expectation(i)
    upload(ctx, k)
    status, off, out, total = render_device(ctx, i, "ranks")
    np.testing.assert_array_equal(status, [w[0] for w in want])
    assert (status == OK).all()
    assert out[:total].tobytes() == b"".join(w[1] for w in want)
    np.testing.assert_array_equal(np.diff(off), [len(w[1]) for w in want])
    assert (out[total:] == 0xAB).all()
    st_h, anns = ctx.gas_annotations_render_ranks(i["node"], i["ncont"], i["cpc"], i["cards"])
    np.testing.assert_array_equal(st_h, status)
    assert anns == [w[1] for w in want]
    # resolve(render(x)) == x, on the device
    if B == 0:
        return
    verdict = torch.empty(B, dtype=torch.int32, device="cuda")
    listed = torch.empty(B, dtype=torch.int32, device="cuda")
    cpc = torch.empty((B, C), dtype=torch.int32, device="cuda")
    cards = torch.empty((B, i["ld"]), dtype=torch.int32, device="cuda")
    ctx.gas_annotations_resolve_device(
        B, dev(np.arange(B, dtype=np.int32)), dev(i["node"]), B, dev(i["ncont"]), C, total,
        dev(off), dev(out[:max(total, 1)]), i["ld"], verdict, listed, cpc, cards)
    torch.cuda.synchronize()
    held = i["node"] >= 0
    np.testing.assert_array_equal(cpc.cpu().numpy()[held], i["cpc"][held])
    np.testing.assert_array_equal(cards.cpu().numpy()[held], i["cards"][held])
    np.testing.assert_array_equal(listed.cpu().numpy()[held], i["cpc"][held].sum(axis=1))


@pytest.mark.gpu
def test_ranks_form_errors(ctx):
    """A rank outside [0, L), a parked rank, more listed cards than the row holds, a negative
    cards_per_container (reads as 0) and a node outside the snapshot (the device form only)."""
    k, C = 8, 3
    n_cards, rows = table_case(k)
    upload(ctx, k)
    L1 = int(n_cards[1])
    node = np.array([0, 0, 1, 0, 0, 0, N + 3, -1, 0], np.int32)
    ncont = np.array([2, 2, 1, 2, 2, 2, 2, 2, 7], np.int32)  # (7: clamped to C)
    cpc = np.array([[1, 1, 0], [1, 1, 0], [1, 0, 0], [1, 1, 0], [2, 2, 0], [-5, 1, 0],
                    [1, 1, 0], [1, 1, 0], [1, 0, 1]], np.int32)
    cards = np.array([[0, 1, -1], [0, k, -1], [L1, -1, -1], [2, 3, 9], [0, 1, 2], [4, -1, -1],
                      [0, 1, -1], [0, 1, -1], [5, 6, -1]], np.int32)
    want_st = [OK, ERR_INPUT, ERR_INPUT, OK, ERR_INPUT, OK, ERR_INPUT, OK, OK]
    r = rows[0]
    want = [r[0] + b"|" + r[1], b"", b"", r[2] + b"|" + r[3], b"", b"|" + r[4], b"", b"",
            r[5] + b"||" + r[6]]
    i = dict(B=len(node), C=C, node=node, ncont=ncont, cpc=cpc, cards=cards, ld=3)
    status, off, out, total = render_device(ctx, i, "ranks")
    assert status.tolist() == want_st
    assert [out[off[b]:off[b + 1]].tobytes() for b in range(len(node))] == want
    host = [0, 1, 2, 3, 4, 5, 7]  # the host form takes neither the node nor the 7 containers
    st_h, anns = ctx.gas_annotations_render_ranks(node[host], ncont[host], cpc[host], cards[host])
    assert st_h.tolist() == [want_st[b] for b in host] and anns == [want[b] for b in host]
    for bad in ([0, N], [0, -2]):
        with pytest.raises(_lib.PasError) as e:
            ctx.gas_annotations_render_ranks(bad, [1, 1], cpc[:2], cards[:2])
        assert e.value.code == _lib.PAS_EINVAL
    with pytest.raises(_lib.PasError) as e:
        ctx.gas_annotations_render([0], [C + 1], np.zeros((1, C, k), np.int64))
    assert e.value.code == _lib.PAS_EINVAL


@pytest.mark.gpu
def test_counts_form_node_out_of_range_on_the_device(ctx):
    k, C = 8, 3
    _, rows = table_case(k)
    upload(ctx, k)
    counts = np.zeros((3, C, k), np.int64)
    counts[:, 0, 0] = 1
    i = dict(B=3, C=C, node=np.array([0, N, 0], np.int32), ncont=np.array([1, 1, 1], np.int32),
             counts=counts)
    status, off, out, total = render_device(ctx, i, "counts")
    assert status.tolist() == [OK, ERR_INPUT, OK]
    assert out[:total].tobytes() == rows[0][0] * 2 and off.tolist() == [0, total // 2, total // 2,
                                                                      total]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["counts", "ranks"])
def test_capacity_rule(ctx, form):
    i = bind_case(16, 3, 65)
    upload(ctx, 16)
    _, want_off, _, total = render_device(ctx, i, form)
    assert total > 16
    status, off, out, err = render_device(ctx, i, form, cap=total - 1)
    assert isinstance(err, _lib.PasError) and err.code == _lib.PAS_ECAPACITY
    assert err.n_bytes == total and str(total) in str(err)
    np.testing.assert_array_equal(off, want_off)          # offsets and statuses delivered
    assert (status != -9).all() and (out == 0xAB).all()   # ... and no byte written
    status, off, out, got = render_device(ctx, i, form, cap=total)
    assert got == total and (out[total:] == 0xAB).all() and not (out[:total] == 0xAB).all()


@pytest.mark.gpu
def test_table_checks(ctx):
    k = 8
    gen = upload(ctx, k)
    args = ([0], [1], np.zeros((1, 1, k), np.int64))
    ctx.gas_card_names_resize(N + 1, k)
    with pytest.raises(_lib.PasError) as e:
        ctx.gas_annotations_render(*args)
    assert e.value.code == _lib.PAS_EINVAL and "card-name table" in str(e.value)
    ctx.gas_card_names_drop()
    with pytest.raises(_lib.PasError) as e:
        ctx.gas_annotations_render(*args)
    assert e.value.code == _lib.PAS_ENOSNAP
    upload(ctx, k)
    assert ctx.gas_annotations_render(*args)[1] == [b""]
    assert ctx.gas_snapshot_get()[0] == gen + 10  # no generation moves


# ------------------------------------------------------------------ node names

@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 64, 257])
def test_names_render_against_names_get(ctx, n):
    import torch
    names = [b"" if s % 7 == 3 else (b"n\x00" + bytes([0x80 + s]) * (s % 5) + b"-%d" % s) * (
        40 if s == 9 else 1) for s in range(N)]
    ctx.names_set(*pack_blobs(names))
    off, blob = ctx.names_get()
    table = [blob[off[s]:off[s + 1]] for s in range(N)]
    assert table == names
    rng = np.random.default_rng(n)
    base = 1000
    slots = rng.integers(0, N, size=n).astype(np.int32) + base
    if n >= 64:  # a repeat, slots outside the table, a spare slot
        slots[:6] = [base + 9, base + 9, base - 1, -1, base + N, base + 3]
    want = [table[s - base] if 0 <= s - base < N else b"" for s in slots.tolist()]
    assert ctx.names_render(slots, base) == want
    assert ctx.names_render(slots - base) == want or n >= 64  # (slot_base 0: -1 - base is outside)
    total = sum(len(w) for w in want)
    off_t = torch.full((n + 1,), -9, dtype=torch.int64, device="cuda")
    out = torch.full((total + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    if total:
        with pytest.raises(_lib.PasError) as e:
            ctx.names_render_device(n, dev(slots), base, off_t, out, total - 1)
        assert e.value.code == _lib.PAS_ECAPACITY and e.value.n_bytes == total
        torch.cuda.synchronize()
        assert (out == 0xAB).all()
    assert ctx.names_render_device(n, dev(slots), base, off_t, out, total) == total
    torch.cuda.synchronize()
    assert out.cpu().numpy()[:total].tobytes() == b"".join(want)
    assert (out[total:] == 0xAB).all()
    np.testing.assert_array_equal(off_t.cpu().numpy(), np.cumsum([0] + [len(w) for w in want]))


# ------------------------------------------------------------------ end to end

E_N, E_P, E_K = 64, 200, 2
E_SEED = 0xB1D


@functools.lru_cache(maxsize=None)
def cluster():
    """A small cluster on which a batch takes several rounds at k = 2: most nodes full, two
    prioritize metrics, so many pods walk the same order (the recipe of test_place_complete)."""
    from test_shard import make_case
    snap, batch = make_case(E_SEED, E_N, 6, E_P, 5)
    batch.prio["metric"] %= 2
    gs = wl.make_gas_snapshot(E_N, seed=E_SEED, var_cards=True)
    gb = wl.make_gas_batch(E_P, seed=E_SEED)
    rng = np.random.default_rng(E_SEED)
    roomy = rng.random(E_N) < 0.5
    half = rng.integers(0, 2, gs.used.shape) * gs.cap[:, None, :] // 2
    free = np.where(roomy[:, None, None], half, 0)
    gs.used = np.maximum(gs.used, gs.cap[:, None, :] - np.maximum(free, 1))
    gs.used[np.arange(gs.used.shape[1])[None, :] >= gs.n_cards[:, None]] = 0
    k = gs.used.shape[1]
    rows = []
    for n in range(E_N):
        label = go_sort_strings([f"card{c}" for c in range(int(gs.n_cards[n]))])
        rows.append(label + [f"parked{n}"] * (len(label) < k) + [""] * (k - len(label) - 1))
    gs.used.setflags(write=False)
    return snap, batch, gs, gb, rows


@pytest.fixture(scope="module")
def ctx2():
    c = pas_amd.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_place_to_completion_annotated(ctx, ctx2):
    from pas_amd.placement import AnnotatedPlacement, PlacementResult, place_to_completion
    from test_shard import _dev, _rule_tensors
    snap, batch, gs, gb, rows = cluster()
    k = gs.used.shape[1]
    names = NODE_NAMES[:E_N]
    _gen[0] += 100
    gen = _gen[0]

    def fresh(c):
        c.gas_snapshot_set(gen, gs.n_cards, gs.cap, np.array(gs.used))
        c.gas_card_names_set(E_N, k, *pack_names([c for row in rows for c in row]))
        c.names_set(*pack_names(names))
    ctx.tas_snapshot_set(gen - 1, snap.v_milli, snap.present)
    fresh(ctx)
    rules_t, off_t, prio_t, _ = _rule_tensors(batch, None)
    C = gb.req.shape[1]
    args = (gen - 1, gen, E_P, len(batch.rules), rules_t, off_t, prio_t, None, C, wl.I915,
            _dev(np.array(gb.req)), _dev(np.array(gb.req_mask).view(np.int32)),
            _dev(gb.n_containers), E_K)
    r = place_to_completion(ctx, *args, annotate=True)
    assert isinstance(r, AnnotatedPlacement) and r._fields[:6] == PlacementResult._fields
    node, rnd = r.node.cpu().numpy(), r.round.cpu().numpy()
    assert r.rounds >= 3 and 20 <= r.n_placed < E_P and (rnd > 0).sum() >= 5
    _, used = ctx.gas_snapshot_get()
    assert (r.status.cpu().numpy() == OK).all()
    ann_off, node_off = r.ann_off.cpu().numpy(), r.node_off.cpu().numpy()
    ann, nn = r.ann_bytes.cpu().numpy().tobytes(), r.node_bytes.cpu().numpy().tobytes()
    got_ann = [ann[ann_off[p]:ann_off[p + 1]].decode() for p in range(E_P)]
    got_node = [nn[node_off[p]:node_off[p + 1]].decode() for p in range(E_P)]
    assert got_node == [names[n] if n >= 0 else "" for n in node.tolist()]
    # the pod-after-pod loop on the second context, in the order the rounds bound the pods
    fresh(ctx2)
    order = [p for p in np.lexsort((np.arange(E_P), rnd)).tolist() if node[p] >= 0]
    g2 = gen
    for p in order:
        _, st, cnt = ctx2.gas_bind(g2, g2 + 1, [p], [node[p]], gb.req, gb.req_mask,
                                   gb.n_containers, wl.I915, counts=True)
        g2 += 1
        assert st[0] == OK
        label = rows[node[p]][:int(gs.n_cards[node[p]])]
        assert got_ann[p] == annotation_counts(cnt[0, :, :len(label)], int(gb.n_containers[p]),
                                               label), p
    np.testing.assert_array_equal(ctx2.gas_snapshot_get()[1], used)
    assert all(got_ann[p] == "" for p in range(E_P) if node[p] < 0)
    assert any("," in a for a in got_ann) and any("|" in a for a in got_ann)
    # the strings as ADD events on a fresh snapshot: the placed usage again
    fresh(ctx2)
    st = ctx2.gas_apply_annotations_names(
        gen, gen + 1, np.full(len(order), _lib.PAS_GAS_EV_ADD, np.int32),
        np.array(order, np.int32), *pack_names([got_node[p] for p in order]), gb.req,
        gb.req_mask, gb.n_containers, *pack_names([got_ann[p] for p in order]))
    assert (st == OK).all()
    np.testing.assert_array_equal(ctx2.gas_snapshot_get()[1], used)
    # without annotate: the type and the fields of before
    fresh(ctx)
    plain = place_to_completion(ctx, *args)
    assert type(plain) is PlacementResult
    np.testing.assert_array_equal(plain.node.cpu().numpy(), node)


# ------------------------------------------------------------------ the extender

@pytest.mark.gpu
def test_extender_bind_over_the_resident_table(ctx, ctx2):
    """GASExtender.bind renders through the card-name table: the same bodies and the same
    stored annotation as the host route, on the pods of the extender tests."""
    import copy

    import test_extender as te
    from pas_amd.extender import GASExtender
    from pas_amd.snapshot import gas_snapshot_from_nodes, pack_card_names
    names, nodes = te.gas_cluster()
    kinds = ["gpu.intel.com/i915", "gpu.intel.com/memory.max"]
    n_cards, cap, used, card_names = gas_snapshot_from_nodes(nodes, kinds)
    pods = {("default", f"p{i}"): te.gas_pod(f"p{i}") for i in range(3)}
    pods[("default", "two")] = te.gas_pod("two", mem="2G", i915="2")      # "card0,card1"
    both = te.gas_pod("both", mem="1G")
    both["spec"]["containers"] *= 2                                       # two segments
    pods[("default", "both")] = both
    # the node has two cards of one i915 each: every sequence starts from the empty node
    sequences = [[("two", "node-1"), ("p0", "node-1")],
                 [("both", "node-1")],
                 [("p0", "node-1"), ("p1", "node-1"), ("p2", "node-1"), ("p0", "node-2"),
                  ("nope", "node-1"), ("p1", "node-9")]]
    results = []
    for c, device in ((ctx, True), (ctx2, False)):
        got = []
        for binds in sequences:
            _gen[0] += 100
            c.gas_snapshot_set(_gen[0], n_cards, cap, used)
            if device:
                c.gas_card_names_set(len(names), used.shape[1],
                                     *pack_card_names(card_names, None, used.shape[1]))
            mine = copy.deepcopy(pods)
            ext = GASExtender(c, _gen[0], names, [] if device else card_names, kinds, mine,
                              device_annotations=device)
            bodies = [ext.bind(json.dumps({"PodName": p, "PodNamespace": "default",
                                           "PodUID": "", "Node": n}).encode()) for p, n in binds]
            got.append((bodies, {key[1]: (p["metadata"].get("annotations") or {}).get(
                "gas-container-cards") for key, p in mine.items()}))
        results.append(got)
    assert results[0] == results[1]
    assert results[0][0][1]["two"] == "card0,card1" and results[0][0][0][1][0] == 404
    assert results[0][1][1]["both"] == "card0|card1"
    assert [s for s, _ in results[0][2][0]] == [200, 200, 404, 404, 404, 404]
