"""The resident node-name table (csrc/name_table.hip): set, lookup, first-seen assignment,
resize and remap, each through the host form and the _device form, against a dict model
written here (slot list + dict: TasCache._flush's slot choice and the compact map restated).
The table is never its own yardstick."""
import random

import numpy as np
import pytest
import torch

import pas_amd
from pas_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, ENOSNAP, ECAPACITY = _lib.PAS_EINVAL, _lib.PAS_ENOSNAP, _lib.PAS_ECAPACITY


# ------------------------------------------------------------------ the model
class Model:
    """names[slot] = the slot's name (bytes), b"" for a spare slot."""

    def __init__(self, names):
        self.names = [bytes(n) for n in names]
        self.index = {n: i for i, n in enumerate(self.names) if n}
        assert len(self.index) == sum(1 for n in self.names if n)

    def resolve(self, entries):
        return [self.index.get(e, -1) if e else -1 for e in entries]

    def assign(self, entries, new_cap):
        """(slots, new_entry, new_slot, n_new, ok): ok False changes nothing."""
        new = list(dict.fromkeys(e for e in entries if e and e not in self.index))
        spare = [i for i, n in enumerate(self.names) if not n]
        if len(new) > min(len(spare), new_cap):
            return self.resolve(entries), [], [], len(new), False
        for name, slot in zip(new, spare):
            self.names[slot] = name
            self.index[name] = slot
        return (self.resolve(entries), [entries.index(name) for name in new],
                spare[:len(new)], len(new), True)

    def resize(self, n):
        self.names += [b""] * (n - len(self.names))

    def remap(self, src):
        self.names = [self.names[s] if s >= 0 else b"" for s in src]
        self.index = {n: i for i, n in enumerate(self.names) if n}


def pack(entries):
    off = np.zeros(len(entries) + 1, np.int64)
    np.cumsum([len(e) for e in entries], out=off[1:])
    return off, b"".join(entries)


def on_device(off, blob, pad=0, fill=0):
    big = torch.full((pad + max(len(blob), 1) + pad,), fill, dtype=torch.uint8, device=DEV)
    if blob:
        big[pad:pad + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    return torch.tensor([int(x) for x in off], dtype=torch.int64, device=DEV), big[pad:]


def install(ctx, names):
    ctx.names_set(*pack(names))
    return Model(names)


def table_names(ctx):
    off, blob = ctx.names_get()
    return [blob[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def resolve_device(ctx, off, blob, n_bytes=None, pad=0, fill=0):
    n = len(off) - 1
    off_t, bytes_t = on_device(off, blob, pad, fill)
    slot = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    ctx.names_resolve_device(n, len(blob) if n_bytes is None else n_bytes, off_t, bytes_t, slot)
    ctx.synchronize()
    return slot.cpu().numpy()[:n]


def check_resolve(ctx, model, entries):
    """Both forms against the model."""
    off, blob = pack(entries)
    want = model.resolve(entries)
    assert ctx.names_resolve(off, blob).tolist() == want
    assert resolve_device(ctx, off, blob).tolist() == want


def assign(ctx, form, entries, new_cap=None):
    """names_assign through one form: (slots, new_entry, new_slot, n_new, ok)."""
    off, blob = pack(entries)
    n = len(entries)
    try:
        if form == "host":
            slots, ne, ns = ctx.names_assign(off, blob, new_cap)
        else:
            off_t, bytes_t = on_device(off, blob)
            slot_t = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
            try:
                ne, ns = ctx.names_assign_device(n, len(blob), off_t, bytes_t, slot_t, new_cap)
            finally:
                slots = slot_t.cpu().numpy()[:n]
        return slots.tolist(), ne.tolist(), ns.tolist(), len(ne), True
    except pas_amd.PasError as e:
        assert e.code == ECAPACITY, e
        if form == "host":
            slots = e.slots
        return slots.tolist(), [], [], e.n_new, False


def check_assign(ctx, model, form, entries, new_cap=None):
    got = assign(ctx, form, entries, new_cap)
    want = model.assign(entries, len(entries) if new_cap is None else new_cap)
    assert got == want
    assert table_names(ctx) == model.names
    n_slots, n_named, n_bytes = ctx.names_info()
    assert (n_slots, n_named, n_bytes) == (len(model.names), len(model.index),
                                           sum(len(n) for n in model.names))
    return got


FORMS = ["host", "device"]


def names_with_home(home, buckets, count, prefix):
    out, i = [], 0
    while len(out) < count:
        name = b"%s-%d" % (prefix, i)
        i += 1
        if pas_amd.name_hash(name) & (buckets - 1) == home:
            out.append(name)
    return out


# ------------------------------------------------------------------ no table
def test_every_entry_point_answers_enosnap_without_a_table():
    c = pas_amd.Context(0)
    try:
        off, blob = pack([b"a"])
        calls = [lambda: c.names_info(), lambda: c.names_get(), lambda: c.names_drop(),
                 lambda: c.names_resolve(off, blob), lambda: c.names_assign(off, blob),
                 lambda: c.names_resize(4), lambda: c.names_remap([0]),
                 lambda: resolve_device(c, off, blob),
                 lambda: c.tas_snapshot_update_quantities_names(1, 2, [], [0], [0], b"", [0], b"")]
        for call in calls:
            with pytest.raises(pas_amd.PasError) as e:
                call()
            assert e.value.code == ENOSNAP
        c.names_set(*pack([b"a", b""]))
        assert c.names_info() == (2, 1, 1)
        c.names_drop()
        with pytest.raises(pas_amd.PasError) as e:
            c.names_resolve(off, blob)
        assert e.value.code == ENOSNAP
    finally:
        c.close()


# ------------------------------------------------------------------ table sizes
@pytest.mark.parametrize("n_slots", [0, 1, 1000])
def test_table_sizes(ctx, n_slots):
    rng = random.Random(n_slots)
    names = [b"node-%d-%d" % (i, rng.randrange(10**6)) for i in range(n_slots)]
    model = install(ctx, names)
    assert ctx.names_info() == (n_slots, n_slots, sum(map(len, names)))
    assert table_names(ctx) == names
    absent = [b"other-%d" % i for i in range(max(n_slots, 3))]
    entries = names + absent
    rng.shuffle(entries)
    check_resolve(ctx, model, entries)
    check_resolve(ctx, model, [])
    if n_slots == 0:
        for form in FORMS:
            assert check_assign(ctx, model, form, [b"x"])[3:] == (1, False)


@pytest.mark.parametrize("home", [5, 15])
def test_eight_slots_one_home_bucket(ctx, home):
    """The 8-slot table has 16 buckets.  Eight names with one home bucket form one full probe
    chain; home 15 is the last bucket, so the chain wraps around to bucket 0.  As many absent
    names with the same home walk the whole chain to its end."""
    names = names_with_home(home, 16, 16, b"chain%d" % home)
    present, absent = names[:8], names[8:]
    assert all(pas_amd.name_hash(n) & 15 == home for n in names)
    model = install(ctx, present)
    check_resolve(ctx, model, present + absent)
    check_resolve(ctx, model, absent + present[::-1])
    # the same chain built by assignment instead of set
    for form in FORMS:
        model = install(ctx, [b""] * 8)
        check_assign(ctx, model, form, present[::-1])
        check_resolve(ctx, model, present + absent)


def test_equal_tag_bits(ctx):
    """name_hash.h documents a 32-bit tag (h >> 32).  Two different names with equal tags
    resolve to their own slots; with only one of them in the table, the other (absent, same
    tag) gives -1: the byte compare decides, never the tag."""
    n = 300000
    tags = np.fromiter((pas_amd.name_hash(b"tagged-%d" % i) >> 32 for i in range(n)), np.uint64, n)
    order = np.argsort(tags, kind="stable")
    same = np.flatnonzero(tags[order][1:] == tags[order][:-1])
    assert same.size >= 1, "no pair among 300 000 names (about ten are expected)"
    a, b = (b"tagged-%d" % int(order[same[0] + k]) for k in (0, 1))
    assert a != b and pas_amd.name_hash(a) >> 32 == pas_amd.name_hash(b) >> 32
    model = install(ctx, [b"filler", a, b"", b])
    check_resolve(ctx, model, [a, b, b"filler", b"tagged-x"])
    assert model.resolve([a, b]) == [1, 3]
    model = install(ctx, [a, b""])
    check_resolve(ctx, model, [b, a])
    for form in FORMS:  # the absent one is then first seen and takes the spare slot
        model = install(ctx, [a, b""])
        assert check_assign(ctx, model, form, [b, a, b])[0] == [1, 0, 1]


def test_near_equal_names(ctx):
    names = [b"node-1", b"node-10", b"node-100", b"node-1000", b"rack-a-node-x", b"rack-a-node-y",
             b"rack-a-node-z", b"x" * 64 + b"0", b"x" * 64 + b"1"]
    model = install(ctx, names)
    check_resolve(ctx, model, names[::-1] + [b"node-", b"node-11", b"node-1000 ", b"rack-a-node-",
                                             b"rack-a-node-w", b"x" * 64, b"x" * 64 + b"2",
                                             b"x" * 65 + b"0", b"node"])


def test_name_content(ctx):
    rng = random.Random(300)
    by_length = [bytes(rng.randrange(1, 256) for _ in range(k)) for k in range(1, 301)]
    high = [bytes([0x80 + i, 0xff, 0xfe - i]) for i in range(8)] + ["nœud-é-節點".encode()]
    nul = [b"\0", b"\0\0", b"a\0b", b"a\0", b"a\0\0", b"\0a", b"a"]
    names = list(dict.fromkeys(by_length + high + nul))
    model = install(ctx, names)
    assert table_names(ctx) == names
    entries = names[::-1] + [b"", b"a\0c", b"\0\0\0", bytes([0x80]), by_length[299] + b"!",
                             by_length[299][:-1], b""]
    check_resolve(ctx, model, entries)
    assert model.resolve([b""]) == [-1]


@pytest.fixture(scope="module")
def thousand():
    return [b"worker-%04d.cluster.local" % i for i in range(1000)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_sizes(ctx, thousand, n):
    model = install(ctx, thousand)
    rng = random.Random(n)
    known = [thousand[rng.randrange(1000)] for _ in range(n)]
    unknown = [b"stranger-%d" % i for i in range(n)]
    mixed = [k if rng.random() < 0.5 else u for k, u in zip(known, unknown)]
    for entries in (known, unknown, mixed):
        check_resolve(ctx, model, entries)


def test_device_form_clamps_offsets(ctx):
    """Offsets that are not monotone or lie outside [0, n_bytes]: every span is read clamped.
    The blob's surroundings hold the bytes of known names ("7", "77", "7777"), so a missing
    clamp resolves to a slot where -1 or another slot is due."""
    model = install(ctx, [b"node-7", b"7", b"xy", b"77", b"7777", b"y77", b"node"])
    blob = b"node-7" + b"xy" + b"77"
    nb = len(blob)
    off = [0, 6, 8, 10, 6, -4, 8, nb + 4, nb + 8, 7, 10, 10, -9, -2, 1, 1 << 40, -(1 << 40), 10,
           8, nb + 1, 0]
    entries = []
    for i in range(len(off) - 1):
        b = min(max(off[i], 0), nb)
        e = max(min(max(off[i + 1], 0), nb), b)
        entries.append(blob[b:e])
    want = model.resolve(entries)
    assert sum(w >= 0 for w in want) >= 5 and sum(w < 0 for w in want) >= 5
    got = resolve_device(ctx, off, blob, pad=4096, fill=ord("7"))
    assert got.tolist() == want
    # n_bytes below the blob's length is the bound
    got = resolve_device(ctx, [0, 6, 9, 4], blob, n_bytes=4, pad=4096, fill=ord("7"))
    assert got.tolist() == model.resolve([b"node", b"", b""]) == [6, -1, -1]
    for bad in ([1, 2], [0, 3, 2], [0, -1]):  # the host form rejects such offsets
        with pytest.raises(pas_amd.PasError) as e:
            ctx.names_resolve(bad, blob)
        assert e.value.code == EINVAL


def test_duplicates_at_set(ctx):
    model = install(ctx, [b"keep-0", b"keep-1", b""])
    names = [b"a", b"b", b"dup", b"c", b"", b"dup", b"d", b"", b"e", b"dup", b"f"]
    with pytest.raises(pas_amd.PasError) as e:
        ctx.names_set(*pack(names))
    assert e.value.code == EINVAL and "slot 5 " in str(e.value)
    # the previous table still resolves
    assert table_names(ctx) == model.names
    check_resolve(ctx, model, [b"keep-1", b"dup", b"keep-0", b"a"])
    # two pairs: the lowest losing slot is named; spare slots are no duplicates of each other
    with pytest.raises(pas_amd.PasError) as e:
        ctx.names_set(*pack([b"", b"q", b"p", b"", b"p", b"q", b""]))
    assert "slot 4 " in str(e.value)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.names_set([0, 2, 1], b"ab")
    assert e.value.code == EINVAL
    assert table_names(ctx) == model.names


# ------------------------------------------------------------------ names_assign
@pytest.mark.parametrize("form", FORMS)
def test_assign_takes_spare_slots_in_ascending_order(ctx, form):
    base = [b"n%d" % i for i in range(12)]
    for s in (9, 2, 5, 7):
        base[s] = b""
    model = install(ctx, base)
    got = check_assign(ctx, model, form, [b"n0", b"new-b", b"n3", b"new-a", b"", b"new-b", b"new-c"])
    assert got == ([0, 2, 3, 5, -1, 2, 7], [1, 3, 6], [2, 5, 7], 3, True)
    # nothing new: the lookups only
    assert check_assign(ctx, model, form, [b"new-a", b"n11", b""])[:4] == ([5, 11, -1], [], [], 0)
    assert check_assign(ctx, model, form, [])[:4] == ([], [], [], 0)


@pytest.mark.parametrize("form", FORMS)
def test_assign_repeats_across_waves_and_blocks(ctx, form):
    """A new name first seen at entry 3 and again at 70 (another wave) and 300 (another block):
    one slot, every repeat gets it."""
    model = install(ctx, [b"k%d" % i for i in range(400)] + [b""] * 4)
    entries = [b"k%d" % (i % 400) for i in range(320)]
    for at in (3, 70, 300):
        entries[at] = b"returning"
    entries[200] = entries[310] = b"later"
    got = check_assign(ctx, model, form, entries)
    assert got[1:] == ([3, 200], [400, 401], 2, True)
    assert [got[0][i] for i in (3, 70, 300, 200, 310)] == [400, 400, 400, 401, 401]


@pytest.mark.parametrize("form", FORMS)
def test_assign_600_new_names(ctx, form):
    rng = random.Random(600)
    base = [b"old-%d" % i if rng.random() < 0.5 else b"" for i in range(1500)]
    model = install(ctx, base)
    new = [b"fresh-%d" % i for i in range(600)]
    entries = new + [n for n in base if n][:200] + new[:100]
    rng.shuffle(entries)
    got = check_assign(ctx, model, form, entries)
    assert got[3] == 600 and got[4] and sorted(got[2]) == got[2]


@pytest.mark.parametrize("form", FORMS)
def test_assign_capacity_then_resize(ctx, form):
    model = install(ctx, [b"a", b"", b"b", b""])
    entries = [b"x", b"a", b"y", b"z", b"x"]
    # too few spare slots, then new_cap: n_new is set, nothing changes, the plain lookups
    assert check_assign(ctx, model, form, entries) == ([-1, 0, -1, -1, -1], [], [], 3, False)
    ctx.names_resize(8)
    model.resize(8)
    assert table_names(ctx) == model.names
    assert check_assign(ctx, model, form, entries, new_cap=2) == \
        ([-1, 0, -1, -1, -1], [], [], 3, False)
    check_resolve(ctx, model, entries)
    # the retry succeeds
    assert check_assign(ctx, model, form, entries) == ([1, 0, 3, 4, 1], [0, 2, 3], [1, 3, 4], 3,
                                                      True)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.names_resize(7)
    assert e.value.code == EINVAL


def test_random_sequence_against_the_model(ctx):
    """200 seeded steps of assign / resize / remap over names drawn from a pool of 300: after
    every step names_get equals the model, on one context driven through the host forms and
    on another driven through the _device forms."""
    other = pas_amd.Context(0)
    try:
        rng = random.Random(2024)
        pool = [b"pool-%d" % i + b"x" * (i % 7) for i in range(300)]
        model = Model([b""] * 16)
        for c in (ctx, other):
            c.names_set(*pack(model.names))
        for step in range(200):
            kind = rng.choice(["assign"] * 5 + ["resize", "remap"])
            if kind == "assign":
                entries = [rng.choice(pool) for _ in range(rng.randrange(0, 40))]
                new_cap = rng.choice([None, None, 3])
                want = model.assign(entries, len(entries) if new_cap is None else new_cap)
                for c, form in ((ctx, "host"), (other, "device")):
                    assert assign(c, form, entries, new_cap) == want, (step, form)
            elif kind == "resize":
                n = len(model.names) + rng.randrange(0, 24)
                model.resize(n)
                for c in (ctx, other):
                    c.names_resize(n)
            else:
                keep = [s for s in range(len(model.names)) if rng.random() < 0.7]
                marks = [True] * len(keep) + [False] * rng.randrange(0, 8)
                rng.shuffle(marks)  # the entries >= 0 stay increasing, the -1 fall anywhere
                kept = iter(keep)
                src = [next(kept) if m else -1 for m in marks]
                model.remap(src)
                for c in (ctx, other):
                    c.names_remap(src)
            for c in (ctx, other):
                assert table_names(c) == model.names, (step, kind)
                assert c.names_info()[:2] == (len(model.names), len(model.index))
        probe = pool[::3] + [b"never"]
        check_resolve(ctx, model, probe)
        check_resolve(other, model, probe)
    finally:
        other.close()


def test_resolve_on_another_stream_follows_the_table_change(ctx):
    """A lookup enqueued on a stream of its own after an assignment, a resize and a remap sees
    the table they left (it waits on the change's event, the host does not wait for it)."""
    model = install(ctx, [b"a", b"", b"b", b""])
    side = torch.cuda.Stream()
    entries = [b"new", b"a", b"b", b"gone"]
    off, blob = pack(entries)
    off_t, bytes_t = on_device(off, blob)
    slot = torch.full((len(entries),), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    for change in (lambda: (ctx.names_assign(*pack([b"new"])), model.assign([b"new"], 1)),
                   lambda: (ctx.names_resize(9), model.resize(9)),
                   lambda: (ctx.names_remap([1, -1, 2]), model.remap([1, -1, 2]))):
        change()
        ctx.names_resolve_device(len(entries), len(blob), off_t, bytes_t, slot, stream=side)
        side.synchronize()
        assert slot.tolist() == model.resolve(entries)
    assert model.resolve(entries) == [0, -1, 2, -1]


# ------------------------------------------------------------------ names_remap
def test_remap(ctx):
    names = [b"r%d" % i for i in range(10)]
    names[4] = b""
    model = install(ctx, names)
    src = [0, -1, 2, 4, 5, -1, 9, -1]
    ctx.names_remap(src)
    model.remap(src)
    assert table_names(ctx) == model.names
    assert ctx.names_info() == (8, 4, sum(len(n) for n in model.names))
    # dropped names resolve to -1, kept names to their new slots
    check_resolve(ctx, model, names)
    assert model.resolve([b"r1", b"r9", b"r5"]) == [-1, 6, 4]
    # the -1 entries (and the spare slot that was kept) are spare and are assigned next
    got = check_assign(ctx, model, "host", [b"r1", b"r3", b"fresh", b"r0"])
    assert got == ([1, 3, 5, 0], [0, 1, 2], [1, 3, 5], 3, True)
    for bad in ([1, 1], [2, 1], [0, 10], [-2], [0, -1, 0]):
        with pytest.raises(pas_amd.PasError) as e:
            ctx.names_remap(bad)
        assert e.value.code == EINVAL
    assert table_names(ctx) == model.names
    ctx.names_remap([])
    assert ctx.names_info() == (0, 0, 0)


@pytest.mark.parametrize("n_slots", [63, 64, 65, 257, 600])
def test_remap_across_wave_and_block_edges(ctx, n_slots):
    """Tables of one wave less a lane, one wave, one wave and a lane, a block and a lane, and
    more than two blocks, every third slot spare.  The map keeps every second slot in ascending
    order, with -1 entries at the front, in the middle and at the end: the named count (one
    ballot per wave, a last wave that is not full) and the packed pool against the model."""
    names = [b"" if i % 3 == 2 else b"edge-%d" % i for i in range(n_slots)]
    model = install(ctx, names)
    assert ctx.names_info() == (n_slots, len(model.index), sum(map(len, names)))
    kept = list(range(0, n_slots, 2))
    mid = len(kept) // 2
    src = [-1, -1] + kept[:mid] + [-1] + kept[mid:] + [-1, -1, -1]
    ctx.names_remap(src)
    model.remap(src)
    assert table_names(ctx) == model.names
    assert ctx.names_info() == (len(src), len(model.index), sum(map(len, model.names)))
    check_resolve(ctx, model, names)
    # the lowest spare slots go first: the two -1 entries at the front, then the next spare one
    spare = [j for j, n in enumerate(model.names) if not n]
    assert spare[:2] == [0, 1] and len(spare) > 6
    got = check_assign(ctx, model, "host", [b"fresh-0", names[0], b"fresh-1", b"fresh-2"])
    assert got == ([0, 2, 1, spare[2]], [0, 2, 3], spare[:3], 3, True)


def test_get_with_a_short_buffer(ctx):
    """A buffer one byte short: PAS_ECAPACITY, the offsets are still delivered and the message
    names the byte count (the raw call: Context.names_get sizes its buffer from names_info)."""
    names = [b"short-%d" % i for i in range(65)]
    install(ctx, names)
    n_bytes = sum(map(len, names))
    off = np.zeros(len(names) + 1, np.int64)
    buf = np.zeros(n_bytes, np.uint8)
    rc = ctx._l.pas_names_get(ctx._h, off.ctypes.data, buf.ctypes.data, n_bytes - 1)
    assert rc == ECAPACITY and off[-1] == n_bytes
    assert off.tolist() == pack(names)[0].tolist()
    assert str(n_bytes) in ctx.last_error()


# ------------------------------------------------------------------ scale
def test_hundred_thousand_names(ctx):
    n = 100000
    names = [b"node-%06d.zone-%d.example.net" % (i, i % 7) for i in range(n)]
    model = install(ctx, names)
    rng = random.Random(5)
    entries = names + [b"node-%06d.zone-%d.example.org" % (i, i % 7) for i in range(n // 10)]
    rng.shuffle(entries)
    off, blob = pack(entries)
    want = np.array(model.resolve(entries), np.int32)
    np.testing.assert_array_equal(ctx.names_resolve(off, blob), want)
    off_t = torch.from_numpy(off).to(DEV)
    bytes_t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    slot = torch.full((len(entries),), -7, dtype=torch.int32, device=DEV)
    ctx.names_resolve_device(len(entries), len(blob), off_t, bytes_t, slot)
    ctx.synchronize()
    np.testing.assert_array_equal(slot.cpu().numpy(), want)
    assert (want < 0).sum() == n // 10
