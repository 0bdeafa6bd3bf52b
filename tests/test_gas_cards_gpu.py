"""The resident card-name table (csrc/gas_cards.hip) against a Python model: a list of rows of
k byte strings.  set / get round trips, whole-row updates (a slot given twice keeps the later
row), growth of both sizes, the compact map with dropped and -1 rows, the bound on the byte pool
under repeated updates, and the error paths, which leave the previous table readable."""
import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd.snapshot import pack_names

SHAPES = [(1, 8), (65, 16), (300, 64)]


def model_rows(n_slots, k, seed):
    """Rows of k names: label-like names, some empty, bytes >= 0x80 and a byte 0, and one name
    of 300 bytes."""
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(n_slots):
        row = []
        for c in range(k):
            kind = rng.integers(0, 6)
            row.append(b"" if kind == 0 else b"card%d" % c if kind < 4 else
                       b"\xc3\xa9-%d\x00x" % s if kind == 4 else
                       bytes(rng.integers(0, 256, 5).astype(np.uint8)))
        rows.append(row)
    rows[n_slots // 2][k // 2] = b"L" * 300
    rows[0][0] = b""
    return rows


def flat(rows):
    return [name for row in rows for name in row]


def install(ctx, rows, k):
    ctx.gas_card_names_set(len(rows), k, *pack_names(flat(rows)))


def read(ctx):
    n, k, _ = ctx.gas_card_names_info()
    off, blob = ctx.gas_card_names_get()
    assert len(off) == n * k + 1 and off[0] == 0 and off[-1] == len(blob)
    names = [blob[off[i]:off[i + 1]] for i in range(n * k)]
    return [names[s * k:(s + 1) * k] for s in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots,k", SHAPES)
def test_set_get_round_trip(ctx, n_slots, k):
    rows = model_rows(n_slots, k, 10 * k + n_slots)
    install(ctx, rows, k)
    live = sum(map(len, flat(rows)))
    assert ctx.gas_card_names_info() == (n_slots, k, live)
    assert read(ctx) == rows
    # a buffer one byte short: PAS_ECAPACITY, the offsets are still delivered
    off = np.zeros(n_slots * k + 1, np.int64)
    buf = np.zeros(live, np.uint8)
    rc = ctx._l.pas_gas_card_names_get(ctx._h, off.ctypes.data, buf.ctypes.data, live - 1)
    assert rc == _lib.PAS_ECAPACITY and off[-1] == live
    assert str(live) in ctx.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots,k", SHAPES)
def test_update_resize_remap_against_the_model(ctx, n_slots, k):
    rng = np.random.default_rng(k)
    rows = model_rows(n_slots, k, 3 * k)
    install(ctx, rows, k)
    # whole rows, one slot given twice: the later row stays
    slots = [n_slots - 1, 0, n_slots - 1] if n_slots > 1 else [0, 0]
    new = [[b"u%d-%d" % (r, c) if c % 3 else b"" for c in range(k)] for r in range(len(slots))]
    ctx.gas_card_names_update(slots, *pack_names(flat(new)))
    for r, s in enumerate(slots):
        rows[s] = new[r]
    assert read(ctx) == rows
    # both sizes grow (k only below the largest tier); new entries are empty names
    k2 = min(2 * k, _lib.PAS_GAS_MAX_CARDS)
    n2 = n_slots + 70
    ctx.gas_card_names_resize(n2, k2)
    rows = [row + [b""] * (k2 - k) for row in rows] + [[b""] * k2 for _ in range(70)]
    assert ctx.gas_card_names_info()[:2] == (n2, k2)
    assert read(ctx) == rows
    ctx.gas_card_names_update([n2 - 1], *pack_names([b"tail%d" % c for c in range(k2)]))
    rows[n2 - 1] = [b"tail%d" % c for c in range(k2)]
    # the compact map: rows dropped, -1 rows in between and behind
    keep = sorted(rng.choice(n2, size=max(n2 // 2, 1), replace=False).tolist())
    src = keep[:1] + [-1] + keep[1:] + [-1, -1]
    ctx.gas_card_names_remap(src)
    rows = [rows[s] if s >= 0 else [b""] * k2 for s in src]
    live = sum(map(len, flat(rows)))
    assert ctx.gas_card_names_info() == (len(src), k2, live)  # the pool is gathered
    assert read(ctx) == rows
    # and the table is writable after the remap
    ctx.gas_card_names_update([1], *pack_names([b"again"] * k2))
    rows[1] = [b"again"] * k2
    assert read(ctx) == rows


@pytest.mark.gpu
def test_table_with_no_rows(ctx):
    """No row at all: set, get and remap launch nothing and still answer; the table then grows
    from nothing and takes an update."""
    k = 8
    ctx.gas_card_names_set(0, k, [0], b"")
    assert ctx.gas_card_names_info() == (0, k, 0)
    off, blob = ctx.gas_card_names_get()
    assert off.tolist() == [0] and blob == b""
    ctx.gas_card_names_remap([])
    assert ctx.gas_card_names_info() == (0, k, 0)
    assert read(ctx) == []
    ctx.gas_card_names_resize(3, k)
    rows = [[b""] * k for _ in range(3)]
    assert read(ctx) == rows
    rows[2] = [b"late%d" % c if c % 2 else b"" for c in range(k)]
    ctx.gas_card_names_update([2], *pack_names(rows[2]))
    assert ctx.gas_card_names_info() == (3, k, sum(map(len, rows[2])))
    assert read(ctx) == rows


@pytest.mark.gpu
def test_repeated_updates_do_not_grow_the_pool_without_bound(ctx):
    n_slots, k = 65, 16
    rows = model_rows(n_slots, k, 5)
    install(ctx, rows, k)
    slots = [3, 17, 64]
    for rnd in range(50):
        new = [[b"round%03d-%d-%d" % (rnd, s, c) for c in range(k)] for s in slots]
        ctx.gas_card_names_update(slots, *pack_names(flat(new)))
        for s, row in zip(slots, new):
            rows[s] = row
        live = sum(map(len, flat(rows)))
        one_round = sum(map(len, flat(new)))
        assert ctx.gas_card_names_info()[2] < 2 * live + one_round, rnd
    assert read(ctx) == rows
    # rewriting every row many times passes the threshold: the pool was gathered on the way
    for rnd in range(4):
        ctx.gas_card_names_update(list(range(n_slots)), *pack_names(flat(rows)))
        assert ctx.gas_card_names_info()[2] <= 2 * live
    assert read(ctx) == rows


@pytest.mark.gpu
def test_error_paths_leave_the_table_readable(ctx):
    k = 8
    rows = model_rows(4, k, 99)
    install(ctx, rows, k)

    def refused(call, *args):
        with pytest.raises(pas_amd.PasError) as err:
            call(*args)
        assert err.value.code == _lib.PAS_EINVAL, err.value
        assert read(ctx) == rows

    off, blob = pack_names(flat(rows))
    bad = off.copy()
    bad[3] = bad[2] - 1
    refused(ctx.gas_card_names_set, 4, k, bad, blob)                     # offsets decrease
    refused(ctx.gas_card_names_set, 4, k, off + 1, blob)                 # not from 0
    with pytest.raises(pas_amd.PasError):                                # k out of range
        ctx._check(ctx._l.pas_gas_card_names_set(ctx._h, 4, 65, off.ctypes.data, None), "set")
    with pytest.raises(pas_amd.PasError):
        ctx._check(ctx._l.pas_gas_card_names_set(ctx._h, 4, 0, off.ctypes.data, None), "set")
    assert read(ctx) == rows
    one = pack_names([b"x"] * k)
    refused(ctx.gas_card_names_update, [4], *one)                        # slot out of range
    refused(ctx.gas_card_names_update, [-1], *one)
    refused(ctx.gas_card_names_update, [0, 9], *pack_names([b"x"] * (2 * k)))  # nothing changed
    refused(ctx.gas_card_names_resize, 3, k)                             # sizes only grow
    refused(ctx.gas_card_names_resize, 4, k - 1)
    refused(ctx.gas_card_names_resize, 4, 65)
    refused(ctx.gas_card_names_remap, [1, 0])                            # not increasing
    refused(ctx.gas_card_names_remap, [0, 4])                            # past the table
    refused(ctx.gas_card_names_remap, [-2])
    # without a table every entry point answers PAS_ENOSNAP
    ctx.gas_card_names_drop()
    for call, args in [(ctx.gas_card_names_info, ()), (ctx.gas_card_names_get, ()),
                       (ctx.gas_card_names_update, ([0],) + one),
                       (ctx.gas_card_names_resize, (8, k)), (ctx.gas_card_names_remap, ([0],)),
                       (ctx.gas_card_names_drop, ())]:
        with pytest.raises(pas_amd.PasError) as err:
            call(*args)
        assert err.value.code == _lib.PAS_ENOSNAP, call
    install(ctx, rows, k)  # and a set brings it back
    assert read(ctx) == rows
