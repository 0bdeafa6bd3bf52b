"""pas_tas_snapshot_update_quantities_names against pas_tas_snapshot_update_quantities given
the slots a dict model looks up, on two contexts over the same base snapshot.  The yardstick
is the existing call; the name table never checks itself."""
import numpy as np
import pytest
import torch

import pas_amd
from pas_amd import _lib
from pas_amd import snapshot as sn
from test_ingest_gpu import BACK, M_BASE, assert_same_snapshot, base_snapshot, set_base

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 130          # snapshot nodes: more than one wave, no multiple of 64
N_SLOTS = 140    # the table's slots: the last ten lie past the snapshot's nodes


@pytest.fixture(scope="module")
def other():
    c = pas_amd.Context(0)
    yield c
    c.close()


def table_names():
    names = [f"n{i}" for i in range(N)] + [f"far{i}" for i in range(N_SLOTS - N)]
    names[17] = ""  # a spare slot in the middle
    return names


def cases():
    names = table_names()

    def cyc(vals, step=1):
        return {names[i]: vals[i % len(vals)] for i in range(0, N, step) if names[i]}

    return {
        "milli": {**cyc(["1", "2.5", "100m"]), "ghost0": "7", "far3": "8"},
        "e7": cyc(["1e-7", "1"], 2),
        "mix": {**cyc(["1e-7", "1e12"]), "ghost1": "1e16"},  # turns wide
        "back": cyc(["3", "4"]),                             # wide in the base, narrow again
        "empty": {},
        "outside": {"ghost0": "1", "ghost2": "1e-9", "far0": "1e16", "far9": "7Ki", "n17": "1"},
    }


COLS = {"milli": 0, "e7": 9, "mix": 2, "back": BACK, "empty": 6, "outside": 7}


def by_names(ctx, form, gen, cols, col_off, nodes, lit_off, blob):
    name_off, name_blob = sn.pack_names(nodes)
    if form == "host":
        return ctx.tas_snapshot_update_quantities_names(gen, gen + 1, cols, col_off, name_off,
                                                        name_blob, lit_off, blob)

    def dev(b):
        return torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to(DEV)

    return ctx.tas_snapshot_update_quantities_names_device(
        gen, gen + 1, cols, col_off, len(name_blob), torch.from_numpy(name_off).to(DEV),
        dev(name_blob), len(blob), torch.from_numpy(lit_off).to(DEV), dev(blob))


def both_bases(ctx, other, gen):
    base = base_snapshot(N)
    for c in (ctx, other):
        set_base(c, gen, base)
    names = table_names()
    other.names_set(*sn.pack_names(names))
    return {name: i for i, name in enumerate(names) if name}


@pytest.mark.parametrize("form", ["host", "device"])
def test_names_refresh_equals_slot_refresh(ctx, other, form):
    gen = 9100
    index = both_bases(ctx, other, gen)
    metrics = cases()
    order = ["outside", "mix", "milli", "empty", "back", "e7"]
    cols = [COLS[name] for name in order]
    col_off, nodes, lit_off, blob = sn.pack_literals(metrics, order)
    entry_node = np.array([index.get(x, -1) for x in nodes], np.int32)
    assert (entry_node >= N).sum() == 3 and (entry_node < 0).sum() == 5  # far*, ghost* and n17
    kind_a, scale_a = ctx.tas_snapshot_update_quantities(gen, gen + 1, cols, col_off, entry_node,
                                                         lit_off, blob)
    kind_b, scale_b, unknown = by_names(other, form, gen, cols, col_off, nodes, lit_off, blob)
    assert unknown == 5
    assert kind_a.tolist() == kind_b.tolist() and scale_a.tolist() == scale_b.tolist()
    assert kind_b[order.index("mix")] == 1 and kind_b[order.index("back")] == 0
    assert kind_b[order.index("outside")] == 0 and scale_b[order.index("outside")] == 3
    got, want = other.tas_snapshot_get(), ctx.tas_snapshot_get()
    assert got[0] == want[0] == gen + 1
    assert_same_snapshot(got, want)
    outside = np.zeros_like(got[2][COLS["outside"]])
    np.testing.assert_array_equal(got[2][COLS["outside"]], outside)  # no node in range
    # the table itself did not change: lookup only
    assert other.names_info()[:2] == (N_SLOTS, N_SLOTS - 1)
    # n_cols = 0 moves the generation only
    before = other.tas_snapshot_get()
    kind, scale, unknown = by_names(other, form, gen + 1, [], np.zeros(1, np.int64), [],
                                    np.zeros(1, np.int64), b"")
    assert len(kind) == 0 and len(scale) == 0 and unknown == 0
    after = other.tas_snapshot_get()
    assert after[0] == gen + 2
    for x, y in zip(before[1:], after[1:]):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("form", ["host", "device"])
def test_bad_literal_at_an_unknown_name_changes_nothing(ctx, other, form):
    gen = 9200
    both_bases(ctx, other, gen)
    metrics = {"milli": {"n0": "1", "n1": "2"}, "e7": {"n2": "3", "ghost5": "1K", "n3": "1e19"}}
    col_off, nodes, lit_off, blob = sn.pack_literals(metrics, ["milli", "e7"])
    before = [np.asarray(x).tobytes() for x in other.tas_snapshot_get()]
    with pytest.raises(pas_amd.PasError) as e:
        by_names(other, form, gen, [0, 9], col_off, nodes, lit_off, blob)
    assert e.value.code == _lib.PAS_EINVAL and e.value.bad_entry == 3
    assert [np.asarray(x).tobytes() for x in other.tas_snapshot_get()] == before
    assert other.tas_snapshot_info()[0] == gen
    # a stale generation and a column outside the snapshot are the existing call's errors
    with pytest.raises(pas_amd.PasError) as e:
        by_names(other, form, gen + 7, [0, 9], col_off, nodes, lit_off, blob)
    assert e.value.code == _lib.PAS_ESTALE
    with pytest.raises(pas_amd.PasError) as e:
        by_names(other, form, gen, [0, M_BASE], col_off, nodes, lit_off, blob)
    assert e.value.code == _lib.PAS_EINVAL
