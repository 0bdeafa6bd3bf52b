"""TasCache(device_names=True): node names are resolved and first-seen nodes get their slots
on the device (the context's resident name table).  GPU: a cache of today's kind
(device_ingest=True) and one with device_names=True, on two contexts, are fed one sequence and
hold the same snapshot and the same cache state after every step.  CPU: the argument checks,
snapshot.pack_names, and the planned calls pinned with a recording stub context."""
import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd import snapshot as sn
from pas_amd.tas_cache import TasCache
from test_tas_cache_ingest import RecordingCtx, assert_same


def table_names(ctx):
    off, blob = ctx.names_get()
    return [blob[off[i]:off[i + 1]].decode() or None for i in range(len(off) - 1)]


@pytest.mark.gpu
def test_two_caches_one_sequence_with_device_names(ctx):
    other = pas_amd.Context(0)
    try:
        start = {"cpu": {"a": "1", "b": "2.5", "c": "100m"}, "temp": {"a": "70", "c": "71"},
                 "idle": {}}
        old = TasCache.from_metrics(ctx, 500, start, device_ingest=True)
        new = TasCache.from_metrics(other, 500, start, device_ingest=True, device_names=True)
        assert new.device_names and not old.device_names

        def same():
            assert_same(old, new)
            assert table_names(other) == new.node_names
            assert new.node_index == {n: i for i, n in enumerate(new.node_names) if n is not None}
            assert other.names_info()[0] == other.tas_snapshot_info()[1] == len(new.node_names)

        def both(method, *args):
            out = [getattr(tc, method)(*args) for tc in (old, new)]
            assert out[0] == out[1]
            same()

        same()
        # the sequence of test_two_caches_one_sequence
        for name in ("cpu", "temp", "ratio", "bytes"):
            both("write_metric", name)
        both("update_all_metrics", lambda name: {
            "cpu": {"a": "1.5", "b": "2", "c": "3"}, "temp": {"a": "69", "b": "70", "c": "72"},
            "ratio": {"a": "0.25", "c": "1e-7"}, "bytes": {"b": "1e12"}, "idle": {"a": "5"}}[name])
        assert not any(new.wide)
        both("write_metric", "power")
        both("update_all_metrics", lambda name: {
            "cpu": {"a": "1", "d": "4", "e": "250m"}, "temp": {"e": "70"},
            "ratio": {"a": "0.5"}, "bytes": {"b": "1e12", "d": "2e12"},
            "power": {n: str(100 + i) for i, n in enumerate("abcdefgh")}, "idle": {}}[name])
        assert "h" in new.node_index and "power" in new.metric_index
        both("write_metric", "bytes", {"a": "1e16", "b": "1"})
        assert new.wide[new.metric_index["bytes"]]
        both("write_metric", "ratio", {"a": "1e-7", "b": "1e12"})
        both("write_metric", "bytes", {"a": "1e6", "b": "1.0001"})
        assert not new.wide[new.metric_index["bytes"]]
        assert new.scale[new.metric_index["bytes"]] == 4

        def fetch(name):
            if name == "cpu":
                raise RuntimeError("metrics API")
            return {}
        both("update_all_metrics", fetch)
        both("delete_metric", "ratio")
        both("delete_metric", "ratio")
        # a refresh with one unparseable value leaves cache, snapshot and table as they were
        before = [np.asarray(x).tobytes() for x in other.tas_snapshot_get()]
        state = (dict(new.data), list(new.scale), list(new.wide), new.gen, list(new.node_names))
        for bad, code in (({"a": "1", "zz": "1K", "b": "2"}, _lib.PAS_EINVAL),
                          ({"a": "1e19", "new-node": "3"}, _lib.PAS_ENOTEXACT)):
            for tc in (old, new):
                with pytest.raises(pas_amd.PasError) as e:
                    tc.write_metric("power", bad)
                assert e.value.code == code
            same()
            assert [np.asarray(x).tobytes() for x in other.tas_snapshot_get()] == before
            assert (new.data, new.scale, new.wide, new.gen, new.node_names) == state
        both("write_metric", "power", {"a": "1", "new-node": "3"})
        assert "new-node" in new.node_index
        # an empty node name: ValueError, nothing changed
        with pytest.raises(ValueError):
            new.write_metric("power", {"a": "2", "": "3"})
        same()

        # 200 first-seen nodes: the table and the snapshot grow
        n_before = len(new.node_names)
        crowd = {f"crowd-{i:03d}": str(i) for i in range(200)}
        both("write_metric", "cpu", {**crowd, "a": "7", "nœud-é": "1.5"})
        assert len(new.node_names) >= n_before + 128 and len(new.node_index) > 202
        assert new.node_index["nœud-é"] > 0
        # a compact drops what no map lists any more; then a dropped node returns
        both("write_metric", "cpu", {"a": "1", "crowd-150": "2", "b": "3"})
        both("compact", None, 3)
        assert "crowd-007" not in new.node_index and len(new.node_names) < n_before + 20
        both("write_metric", "temp", {"crowd-007": "55", "a": "66", "crowd-150": "1"})
        assert new.node_index["crowd-007"] == old.node_index["crowd-007"]
        both("update_all_metrics", lambda name: {"x%d" % i: "1" for i in range(5)})
    finally:
        other.close()


# ------------------------------------------------------------------ CPU
class NamesCtx(RecordingCtx):
    """RecordingCtx plus a dict model of the name table's calls."""

    def __init__(self, names):
        super().__init__()
        self.names = list(names)

    def names_assign(self, name_off, blob, new_cap=None, want_slots=True):
        entries = [blob[name_off[i]:name_off[i + 1]].decode() for i in range(len(name_off) - 1)]
        self.calls.append(("names_assign", entries))
        known = {n for n in self.names if n}
        new = list(dict.fromkeys(e for e in entries if e not in known))
        spare = [i for i, n in enumerate(self.names) if not n]
        if len(new) > len(spare):
            err = pas_amd.PasError(_lib.PAS_ECAPACITY, "pas_names_assign")
            err.n_new = len(new)
            raise err
        for name, slot in zip(new, spare):
            self.names[slot] = name
        return (None, np.array([entries.index(x) for x in new], np.int32),
                np.array(spare[:len(new)], np.int32))

    def names_resize(self, n_slots, stream=None):
        self.calls.append(("names_resize", n_slots))
        self.names += [None] * (n_slots - len(self.names))

    def names_remap(self, src_slot, stream=None):
        self.calls.append(("names_remap", [int(s) for s in src_slot]))
        self.names = [self.names[s] if s >= 0 else None for s in src_slot]

    def tas_snapshot_compact(self, gen_from, gen_to, src_node, stream=None):
        self.calls.append(("compact", gen_from, gen_to, [int(s) for s in src_node]))

    def tas_snapshot_update_quantities(self, *args):
        raise AssertionError("device_names: the refresh goes by names")

    def tas_snapshot_update_quantities_names(self, gen_from, gen_to, cols, col_off, name_off,
                                             name_blob, lit_off, blob):
        self.calls.append(("update_quantities_names", gen_from, gen_to, list(cols),
                           [int(x) for x in col_off], bytes(name_blob), bytes(blob)))
        return np.zeros(len(cols), np.int32), np.full(len(cols), 3, np.int32), 0


class CountingDict(dict):
    """A dict that counts its lookups."""
    probes = 0

    def __getitem__(self, k):
        self.probes += 1
        return dict.__getitem__(self, k)

    def __contains__(self, k):
        self.probes += 1
        return dict.__contains__(self, k)

    def get(self, k, default=None):
        self.probes += 1
        return dict.get(self, k, default)


def test_device_names_argument_checks():
    ctx = NamesCtx(["a"])
    with pytest.raises(ValueError):
        TasCache(ctx, 1, ["a"], ["m"], device_names=True)
    with pytest.raises(ValueError):
        TasCache(ctx, 1, ["a"], ["m"], device_ingest=True, device_names=True,
                 slots=TasCache(ctx, 1, ["a"], ["m"]))
    for kw in ({"device_names": True}, {"device_names": True, "device_ingest": True,
                                        "slots": TasCache(ctx, 1, ["a"], ["m"])}):
        with pytest.raises(ValueError):
            TasCache.from_metrics(ctx, 1, {"m": {"a": "1"}}, **kw)
    assert ctx.calls == []
    assert TasCache(ctx, 1, ["a"], ["m"], device_ingest=True).device_names is False
    # an empty node name: before anything changes, the maps put back
    tc = TasCache(ctx, 1, ["a"], ["m"], device_ingest=True, device_names=True)
    tc.data["m"] = {"a": "1"}
    tc.write_metric("m")
    with pytest.raises(ValueError):
        tc.write_metric("m", {"a": "2", "": "3"})
    with pytest.raises(ValueError):
        tc.update_all_metrics(lambda name: {"": "1"})
    assert ctx.calls == [] and tc.data == {"m": {"a": "1"}} and tc.gen == 1


def test_pack_names():
    off, blob = sn.pack_names(["node-1", "n", "", "node-10"])
    assert off.dtype == np.int64 and off.tolist() == [0, 6, 7, 7, 14] and blob == b"node-1nnode-10"
    off, blob = sn.pack_names([])
    assert off.tolist() == [0] and blob == b""
    names = ["nœud", "a", "節點-1", ""]
    off, blob = sn.pack_names(names)
    assert [blob[off[i]:off[i + 1]].decode() for i in range(4)] == names
    assert off.tolist() == [0, 5, 6, 14, 14]
    off, blob = sn.pack_names(["a", None, b"\xff\x00", "b"])
    assert off.tolist() == [0, 1, 1, 3, 4] and blob == b"a\xff\x00b"


def test_device_names_plans_one_assign_and_one_update():
    ctx = NamesCtx(["a", "b"])
    tc = TasCache(ctx, 100, ["a", "b"], ["m0"], device_ingest=True, device_names=True)
    tc.data["m0"] = {"a": "1"}
    for name in ("m0", "m1", "mw"):
        tc.write_metric(name)
    assert ctx.calls == []
    refresh = {"m0": {"a": "1.000001", "b": "2", "c": "3"}, "m1": {"a": "5"},
               "mw": {"a": "0.0000001", "b": "1000000000000"}}
    tc.update_all_metrics(refresh.__getitem__)
    blob = b"1.000001" b"2" b"3" b"5" b"0.0000001" b"1000000000000"
    entries = ["a", "b", "c", "a", "a", "b"]
    assert ctx.calls == [
        ("parse", 6, blob),
        ("names_assign", entries), ("names_resize", 66), ("names_assign", entries),
        ("reshape", 100, 101, 66, 9),
        ("update_quantities_names", 101, 102, [0, 1, 2], [0, 3, 4, 6], b"abcaab", blob)]
    assert tc.gen == 102 and tc.node_index["c"] == 2 and tc.node_names == ctx.names
    # steady state: one parse, one names_assign, one update, and no dictionary probe per entry
    del ctx.calls[:]
    tc.node_index = CountingDict(tc.node_index)
    tc.update_all_metrics(refresh.__getitem__)
    assert [c[0] for c in ctx.calls] == ["parse", "names_assign", "update_quantities_names"]
    assert tc.node_index.probes == 0 and tc.gen == 103
    # a first-seen node with a spare slot left: no resize, no reshape
    del ctx.calls[:]
    tc.write_metric("m1", {"a": "5", "d": "6"})
    assert [c[0] for c in ctx.calls] == ["parse", "names_assign", "update_quantities_names"]
    assert tc.node_index.probes == 0 and tc.node_names[3] == "d" and tc.node_index["d"] == 3
    # a literal that cannot be held: the parse, nothing else
    del ctx.calls[:]
    with pytest.raises(pas_amd.PasError):
        tc.write_metric("m1", {"a": "1x", "q": "1"})
    assert [c[0] for c in ctx.calls] == ["parse"] and "q" not in dict(tc.node_index)
    # compact applies its map to the table as well
    del ctx.calls[:]
    src = tc.compact(spare_nodes=2)
    assert src == [0, 1, 2, 3, -1, -1]
    assert ctx.calls == [("compact", tc.gen - 1, tc.gen, src), ("names_remap", src)]
    assert tc.node_names == ctx.names
