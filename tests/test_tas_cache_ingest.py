"""TasCache(device_ingest=True): Quantity strings go to the device as they are.  Two caches
on two contexts, one of today's kind, are fed the same sequence; after every step both hold
the same snapshot and the same cache state.  A CPU test pins the calls device_ingest plans."""
import numpy as np
import pytest

import pas_amd
from helpers import unpack_bits
from pas_amd import _lib
from pas_amd.tas_cache import TasCache


def assert_same(a: TasCache, b: TasCache):
    """Equal pas_tas_snapshot_get contents (present bits, values and nanos where present, wide
    marks, scales of the narrow columns) and equal cache state."""
    _, va, pa, sa, wa, na = a.ctx.tas_snapshot_get()
    _, vb, pb, sb, wb, nb = b.ctx.tas_snapshot_get()
    np.testing.assert_array_equal(pa, pb)
    np.testing.assert_array_equal(wa, wb)
    bits = unpack_bits(pa, va.shape[1])
    np.testing.assert_array_equal(va[bits], vb[bits])
    np.testing.assert_array_equal(na[bits], nb[bits])
    np.testing.assert_array_equal(sa[wa == 0], sb[wb == 0])
    assert a.scale == b.scale and a.wide == b.wide and a.counts == b.counts
    assert a.data == b.data
    assert a.node_names == b.node_names and a.metric_names == b.metric_names
    # each cache describes its own snapshot
    for tc, s, w in ((a, sa, wa), (b, sb, wb)):
        assert tc.ctx.tas_snapshot_info()[0] == tc.gen
        assert [bool(x) for x in w] == tc.wide
        assert [int(x) for x, wide in zip(s, w) if not wide] == \
            [x for x, wide in zip(tc.scale, tc.wide) if not wide]


@pytest.mark.gpu
def test_two_caches_one_sequence(ctx):
    other = pas_amd.Context(0)
    try:
        start = {"cpu": {"a": "1", "b": "2.5", "c": "100m"}, "temp": {"a": "70", "c": "71"},
                 "idle": {}}
        old = TasCache.from_metrics(ctx, 500, start)
        new = TasCache.from_metrics(other, 500, start, device_ingest=True)
        assert new.device_ingest and not old.device_ingest
        assert_same(old, new)

        def both(method, *args):
            for tc in (old, new):
                getattr(tc, method)(*args)
            assert_same(old, new)

        # first data for registered names
        for name in ("cpu", "temp", "ratio", "bytes"):
            both("write_metric", name)
        both("update_all_metrics", lambda name: {
            "cpu": {"a": "1.5", "b": "2", "c": "3"}, "temp": {"a": "69", "b": "70", "c": "72"},
            "ratio": {"a": "0.25", "c": "1e-7"}, "bytes": {"b": "1e12"}, "idle": {"a": "5"}}[name])
        assert new.wide == old.wide and not any(new.wide)
        # a refresh that adds nodes and a metric
        both("write_metric", "power")
        both("update_all_metrics", lambda name: {
            "cpu": {"a": "1", "d": "4", "e": "250m"}, "temp": {"e": "70"},
            "ratio": {"a": "0.5"}, "bytes": {"b": "1e12", "d": "2e12"},
            "power": {n: str(100 + i) for i, n in enumerate("abcdefgh")}, "idle": {}}[name])
        assert "h" in new.node_index and "power" in new.metric_index
        # a column turning wide and back
        both("write_metric", "bytes", {"a": "1e16", "b": "1"})
        assert new.wide[new.metric_index["bytes"]]
        both("write_metric", "ratio", {"a": "1e-7", "b": "1e12"})
        assert new.wide[new.metric_index["ratio"]]
        both("write_metric", "bytes", {"a": "1e6", "b": "1.0001"})
        assert not new.wide[new.metric_index["bytes"]]
        assert new.scale[new.metric_index["bytes"]] == 4
        # an empty result keeps the data; a raise too
        def fetch(name):
            if name == "cpu":
                raise RuntimeError("metrics API")
            return {}
        both("update_all_metrics", fetch)
        # a delete
        both("delete_metric", "ratio")
        both("delete_metric", "ratio")
        # a refresh with one unparseable value leaves both as they were
        before = [np.asarray(x).tobytes() for x in other.tas_snapshot_get()]
        state = (dict(new.data), list(new.scale), list(new.wide), new.gen, list(new.node_names))
        for bad, code, lit in (({"a": "1", "zz": "1K", "b": "2"}, _lib.PAS_EINVAL, "1K"),
                               ({"a": "1e19", "new-node": "3"}, _lib.PAS_ENOTEXACT, "1e19")):
            for tc in (old, new):
                with pytest.raises(pas_amd.PasError) as e:
                    tc.write_metric("power", bad)
                assert e.value.code == code
            assert "power" in str(e.value) and repr(lit) in str(e.value)  # device_ingest's
            assert_same(old, new)
            assert [np.asarray(x).tobytes() for x in other.tas_snapshot_get()] == before
            assert (new.data, new.scale, new.wide, new.gen, new.node_names) == state
        # and both go on
        both("write_metric", "power", {"a": "1", "new-node": "3"})
        assert "new-node" in new.node_index
    finally:
        other.close()


class RecordingCtx:
    """Records the device calls TasCache plans, in order."""

    def __init__(self):
        self.calls = []

    def tas_snapshot_reshape(self, gen_from, gen_to, n_nodes, n_metrics, src_col=None,
                             stream=None):
        self.calls.append(("reshape", gen_from, gen_to, n_nodes, n_metrics))

    def quantities_to_wide(self, lit_off, blob):
        n = len(lit_off) - 1
        self.calls.append(("parse", n, bytes(blob)))
        status = np.zeros(n, np.int32)
        for i in range(n):
            status[i] = pas_amd.quantity_parse_fixed(blob[lit_off[i]:lit_off[i + 1]])[0]
        return None, None, None, status

    def tas_snapshot_update_quantities(self, gen_from, gen_to, cols, col_off, entry_node, lit_off,
                                       blob):
        self.calls.append(("update_quantities", gen_from, gen_to, list(cols),
                           [int(x) for x in col_off], [int(x) for x in entry_node], bytes(blob)))
        return np.zeros(len(cols), np.int32), np.full(len(cols), 3, np.int32)


def test_device_ingest_plans_one_update():
    """No per-value call; one parse of all literals, at most one reshape, one update."""
    ctx = RecordingCtx()
    tc = TasCache(ctx, 100, ["a", "b"], ["m0"], device_ingest=True)
    tc.data["m0"] = {"a": "1"}
    for name in ("m0", "m1", "mw"):
        tc.write_metric(name)
    assert ctx.calls == []
    tc.update_all_metrics(lambda name: {
        "m0": {"a": "1.000001", "b": "2", "c": "3"}, "m1": {"a": "5"},
        "mw": {"a": "0.0000001", "b": "1000000000000"}}[name])
    blob = b"1.000001" b"2" b"3" b"5" b"0.0000001" b"1000000000000"
    assert ctx.calls == [
        ("parse", 6, blob),
        ("reshape", 100, 101, 66, 9),
        ("update_quantities", 101, 102, [0, 1, 2], [0, 3, 4, 6], [0, 1, 2, 0, 0, 1], blob)]
    assert tc.gen == 102 and tc.node_index["c"] == 2
    # a literal that cannot be held: the parse, nothing else, the maps put back
    data = {k: dict(v) for k, v in tc.data.items()}
    with pytest.raises(pas_amd.PasError) as e:
        tc.update_all_metrics(lambda name: {"m0": {"a": "9", "q": "8"}, "m1": {"a": "1x"},
                                            "mw": {"a": "1"}}[name])
    assert e.value.code == _lib.PAS_EINVAL and "'m1'" in str(e.value) and "'1x'" in str(e.value)
    assert [c[0] for c in ctx.calls[3:]] == ["parse"]
    assert tc.data == data and tc.gen == 102 and "q" not in tc.node_index


def test_default_keeps_todays_calls():
    assert TasCache(RecordingCtx(), 1, ["a"], ["m"]).device_ingest is False
