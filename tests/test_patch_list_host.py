"""pas_label_patch_json_batch: the PATCH bodies of a whole patch list in one host call are the
bodies pas_label_patch_json renders node by node (and the oracle's), back to back.  Host code
in libpas.so, no GPU."""
import ctypes

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from test_labels import random_names


def _masks(rng, s, n):
    """n (add, rem) pairs over s strategies: disjoint, some empty, some full."""
    live = np.uint64((1 << s) - 1)
    add = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) & live
    add |= rng.integers(0, 2, size=n, dtype=np.uint64) & live
    rem = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) & live & ~add
    if n > 3:
        add[0] = rem[0] = 0       # "[]"
        add[1], rem[1] = live, 0  # every strategy added
        add[2], rem[2] = 0, live  # every label removed
    return add, rem


def _batch_raw(names, add, rem, cap):
    """(status, buffer bytes, offsets, total_len) of one call with a buffer of cap bytes."""
    n = len(add)
    arr = (ctypes.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    off = np.full(n + 1, -1, np.int64)
    total = ctypes.c_int64(-1)
    buf = ctypes.create_string_buffer(max(cap, 1))
    rc = pas_amd.LIB.pas_label_patch_json_batch(
        len(names), arr, n, add.ctypes.data_as(ctypes.c_void_p),
        rem.ctypes.data_as(ctypes.c_void_p), buf, cap, off.ctypes.data_as(ctypes.c_void_p),
        ctypes.byref(total))
    return rc, buf.raw[:cap], off, total.value


@pytest.mark.parametrize("s", [0, 1, 7, 64])
@pytest.mark.parametrize("n", [0, 1, 1000])
def test_batch_equals_per_node_bodies(oracle, s, n):
    rng = np.random.default_rng(100 * s + n)
    names = random_names(rng, s)
    add, rem = _masks(rng, s, n)
    got = pas_amd.label_patch_json_batch(names, add, rem)
    assert len(got) == n
    for i in range(n):
        want = pas_amd.label_patch_json(names, int(add[i]), int(rem[i]))
        assert got[i] == want, (s, i)
        if i < 50:
            assert got[i] == oracle.label_patch_json(names, int(add[i]), int(rem[i]))
    # the raw call: offsets monotone, from 0 to total_len, the bodies back to back
    rc, raw, off, total = _batch_raw(names, add, rem, sum(len(b) for b in got))
    assert rc == _lib.PAS_OK
    assert off[0] == 0 and off[n] == total == len(raw) and np.all(np.diff(off) >= 2)
    assert raw == b"".join(got)


def test_batch_capacity_reports_full_sizes():
    rng = np.random.default_rng(7)
    names = random_names(rng, 7)
    add, rem = _masks(rng, 7, 40)
    _, full, off_full, total_full = _batch_raw(names, add, rem, 1 << 16)
    full = full[:total_full]
    for cap in (0, 1, total_full // 2, total_full - 1):
        rc, raw, off, total = _batch_raw(names, add, rem, cap)
        assert rc == _lib.PAS_ECAPACITY
        assert total == total_full and np.array_equal(off, off_full)
        assert raw == full[:cap]  # what fits is the beginning of the full output
    rc, raw, off, total = _batch_raw(names, add, rem, total_full)
    assert rc == _lib.PAS_OK and raw == full


def test_batch_errors():
    names = ["alpha", "beta"]
    one = np.array([1], np.uint64)
    zero = np.array([0], np.uint64)
    past = np.array([4], np.uint64)  # bit 2 of two strategies
    for add, rem in ((past, zero), (zero, past), (np.array([1, 4], np.uint64),
                                                  np.array([0, 0], np.uint64))):
        rc, raw, off, total = _batch_raw(names, add, rem, 256)
        assert rc == _lib.PAS_EINVAL
        assert raw == b"\0" * 256 and np.all(off == -1) and total == -1  # nothing written
    with pytest.raises(pas_amd.PasError) as e:
        pas_amd.label_patch_json_batch(names, past, zero)
    assert e.value.code == _lib.PAS_EINVAL
    assert _batch_raw([f"n{i}" for i in range(65)], one, zero, 256)[0] == _lib.PAS_EINVAL
    # null output arguments
    arr = (ctypes.c_char_p * 2)(b"alpha", b"beta")
    n = ctypes.c_int64()
    lib = pas_amd.LIB
    p = one.ctypes.data_as(ctypes.c_void_p)
    off = np.zeros(2, np.int64).ctypes.data_as(ctypes.c_void_p)
    assert lib.pas_label_patch_json_batch(2, arr, 1, p, p, None, 8, off, ctypes.byref(n)) == \
        _lib.PAS_EINVAL
    assert lib.pas_label_patch_json_batch(2, arr, 1, p, p, None, 0, None, ctypes.byref(n)) == \
        _lib.PAS_EINVAL
    assert lib.pas_label_patch_json_batch(2, arr, 1, None, p, None, 0, off, ctypes.byref(n)) == \
        _lib.PAS_EINVAL
    # counting only: no buffer, cap 0
    assert lib.pas_label_patch_json_batch(2, arr, 1, p, p, None, 0, off, ctypes.byref(n)) == \
        _lib.PAS_ECAPACITY
    assert n.value == len(pas_amd.label_patch_json(names, 1, 1))
