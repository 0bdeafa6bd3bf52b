"""The render side of the "gas-container-cards" grammar (csrc/annotation_fixed.h) on the CPU:
pas_gas_annotation_render, the host pin of the routine the device runs per bind
(csrc/gas_render.hip, tests/test_gas_render_gpu.py), against snapshot.annotation_counts, the
host restatement of bindNode (scheduler.go:317-335), and back through pas_gas_annotation_parse."""
import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd.context import gas_annotation_parse, gas_annotation_render
from pas_amd.snapshot import annotation_counts

OK, ERR_INPUT, ERR_OVERFLOW = _lib.PAS_GAS_OK, _lib.PAS_GAS_ERR_INPUT, _lib.PAS_GAS_ERR_OVERFLOW
INT32_MAX = 2**31 - 1

NEW_SYMBOLS = [
    "pas_gas_annotation_render", "pas_gas_annotations_render", "pas_gas_annotations_render_device",
    "pas_gas_annotations_render_ranks", "pas_gas_annotations_render_ranks_device",
    "pas_names_render", "pas_names_render_device",
]


def test_new_symbols_present_and_bound():
    lib = pas_amd.LIB
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    for host in ("pas_gas_annotations_render", "pas_gas_annotations_render_ranks",
                 "pas_names_render"):  # the _device forms add the stream
        assert len(_lib.SIGNATURES[host + "_device"][1]) == len(_lib.SIGNATURES[host][1]) + 1
    with open(_lib.HEADER_PATH) as f:
        assert "#define PAS_ABI_VERSION 3" in f.read()  # additions only
    for method in ("gas_annotations_render", "gas_annotations_render_device",
                   "gas_annotations_render_ranks", "gas_annotations_render_ranks_device",
                   "names_render", "names_render_device"):
        assert callable(getattr(pas_amd.Context, method)), method
    assert pas_amd.gas_annotation_render is gas_annotation_render


def expect(counts, names):
    return annotation_counts(counts, len(counts), names).encode("utf-8", "surrogateescape")


def encoded(names):
    return [n.encode("utf-8", "surrogateescape") if isinstance(n, str) else n for n in names]


CARDS = ["card0", "card1", "card10", "card2"]

CASES = {
    "no containers": ([], CARDS),
    "one empty container": ([[0, 0, 0, 0]], CARDS),
    "all-empty containers": ([[0, 0, 0, 0]] * 3, CARDS),
    "one card": ([[0, 1, 0, 0]], CARDS),
    "card1 and card10": ([[0, 1, 1, 0], [0, 0, 1, 0]], CARDS),
    "empty first and last": ([[0] * 4, [1, 0, 0, 1], [0] * 4], CARDS),
    "empty middle": ([[1, 0, 0, 0], [0] * 4, [0, 0, 0, 1]], CARDS),
    "counts of 2 and 70": ([[2, 0, 70, 0], [0, 70, 0, 2]], CARDS),
    "an empty card name": ([[1, 1, 1], [0, 1, 1], [0, 2, 0]], ["a", "", "b"]),
    "only the empty name": ([[2], [3]], [""]),
    "eight containers": ([[c % 2, 0, c % 3, 1] for c in range(8)], CARDS),
}


@pytest.mark.parametrize("name", list(CASES))
def test_render_matches_annotation_counts(name):
    counts, names = CASES[name]
    status, raw = gas_annotation_render(counts, names)
    assert status == OK
    assert raw == expect(counts, names)
    # ... and the parser reads back the segments and the listed count that went in
    segs, cpc, listed, spans = gas_annotation_parse(raw)
    assert segs == max(len(counts), 1)
    assert cpc[:len(counts)] == [sum(row) for row in counts]
    assert listed == sum(sum(row) for row in counts)
    want = [n for row in counts for k, n in enumerate(encoded(names)) for _ in range(row[k])]
    assert [raw[b:b + n] for b, n in spans] == want


def test_one_empty_name_alone_is_the_empty_segment():
    """The grammar's one ambiguity, the reference's as well: a segment that lists the empty name
    once renders as no bytes, which Split reads as a segment without cards."""
    assert gas_annotation_render([[1, 0], [0, 1]], ["", "b"]) == (OK, b"|b")
    assert gas_annotation_parse(b"|b")[1] == [0, 1]


def test_fixed_strings():
    assert gas_annotation_render([[0] * 4] * 3, CARDS) == (OK, b"||")
    assert gas_annotation_render([], CARDS) == (OK, b"")
    assert gas_annotation_render([[1, 1, 1]], ["a", "", "b"]) == (OK, b"a,,b")
    assert gas_annotation_render([[0, 1, 1, 0], [1, 0, 0, 0]], CARDS) == (OK, b"card1,card10|card0")
    assert gas_annotation_render([[2], [0]], ["x"]) == (OK, b"x,x|")


def test_opaque_bytes():
    names = [b"\x00", b"a\x00b", b"\xff\xfe", "é".encode(), b"\x80" * 65]
    counts = [[1, 2, 0, 1, 1], [0, 0, 3, 0, 0]]
    status, raw = gas_annotation_render(counts, names)
    assert status == OK
    assert raw == b"|".join(b",".join(n for k, n in enumerate(names) for _ in range(row[k]))
                            for row in counts)


def test_generated_against_reference():
    rng = np.random.default_rng(317)
    for _ in range(300):
        k = int(rng.integers(1, 9))
        names = [f"card{i}" * int(rng.integers(0, 3)) for i in range(k)]
        c = int(rng.integers(0, 5))
        counts = (rng.integers(0, 4, size=(c, k)) * (rng.random((c, k)) < 0.4)).tolist()
        status, raw = gas_annotation_render(counts, names)
        assert (status, raw) == (OK, expect(counts, names)), (counts, names)


def test_error_statuses():
    assert gas_annotation_render([[0, -1, 0, 0]], CARDS) == (ERR_INPUT, b"")
    assert gas_annotation_render([[1, 0, 0, 0], [0, 0, 0, -2**63]], CARDS) == (ERR_INPUT, b"")
    # a count on a slot at or past n_cards: a parked or unused slot
    assert gas_annotation_render([[1, 0, 0, 1]], CARDS, n_cards=3) == (ERR_INPUT, b"")
    assert gas_annotation_render([[1, 0, 1, 0]], CARDS, n_cards=3) == (OK, b"card0,card10")
    assert gas_annotation_render([[1, 0, 0, 0]], CARDS, n_cards=0) == (ERR_INPUT, b"")
    assert gas_annotation_render([[1, 0, 0, 0]], CARDS, n_cards=-1) == (ERR_INPUT, b"")
    assert gas_annotation_render([[0, 0, 0, 0]] * 2, CARDS, n_cards=-1) == (OK, b"|")
    assert gas_annotation_render([[1, 0, 0, 1]], CARDS, n_cards=99) == (OK, b"card0,card2")
    # the input error wins over the length
    assert gas_annotation_render([[2**62, -1, 0, 0]], CARDS) == (ERR_INPUT, b"")


def test_saturation_at_int32_max():
    assert gas_annotation_render([[2**62, 0, 0, 0]], CARDS) == (ERR_OVERFLOW, b"")
    assert gas_annotation_render([[2**63 - 1] * 4] * 8, CARDS) == (ERR_OVERFLOW, b"")
    assert gas_annotation_render([[2**63 - 1]], [""]) == (ERR_OVERFLOW, b"")
    # the edge, by the sizing call alone: count repeats of "" are count - 1 commas
    with pytest.raises(_lib.PasError) as e:
        gas_annotation_render([[2**31]], [""], cap=0)
    assert e.value.code == _lib.PAS_ECAPACITY and e.value.n_bytes == INT32_MAX
    assert gas_annotation_render([[2**31 + 1]], [""], cap=0) == (ERR_OVERFLOW, b"")
    # two containers: INT32_MAX - 1 commas and the bar are INT32_MAX bytes and fit, one more
    # name byte does not
    with pytest.raises(_lib.PasError) as e:
        gas_annotation_render([[2**31 - 1, 0], [0, 0]], ["", "x"], cap=0)
    assert e.value.code == _lib.PAS_ECAPACITY and e.value.n_bytes == INT32_MAX
    assert gas_annotation_render([[2**31 - 1, 0], [0, 1]], ["", "x"], cap=0) == (ERR_OVERFLOW, b"")
    # a name of 5 bytes: 357913941 repeats are 2147483645 bytes, one more repeat is past the end
    with pytest.raises(_lib.PasError) as e:
        gas_annotation_render([[357913941, 0, 0, 0]], CARDS, cap=0)
    assert e.value.n_bytes == 357913941 * 6 - 1
    assert gas_annotation_render([[357913942, 0, 0, 0]], CARDS, cap=0) == (ERR_OVERFLOW, b"")


def test_standalone_program_under_sanitizers(tmp_path):
    """scripts/diag/annotation_render_check.cpp: the header and the host entry point in a
    program of its own (nothing preloaded, nothing loaded into Python), built with ASan +
    UBSan; 20 000 seeded random binds into buffers of exactly the reported size against a
    restated join."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "platform-aware-scheduling_amd", "csrc")
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer build of the host code"
    exe = tmp_path / "annotation_render_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(root, "include"), "-I", csrc,
                    os.path.join(root, "scripts", "diag", "annotation_render_check.cpp"),
                    os.path.join(csrc, "gas_annotation.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.startswith("ok: 20000 random binds")


def test_short_cap():
    counts = [[1, 1, 0, 0], [0, 0, 0, 1]]
    want = expect(counts, CARDS)
    with pytest.raises(_lib.PasError) as e:
        gas_annotation_render(counts, CARDS, cap=len(want) - 1)
    assert e.value.code == _lib.PAS_ECAPACITY and e.value.n_bytes == len(want)
    assert gas_annotation_render(counts, CARDS, cap=len(want)) == (OK, want)
    # the raw call: nothing is written into a short buffer
    l = pas_amd.LIB
    import ctypes
    c = np.array(counts, np.int64)
    off = np.zeros(5, np.int64)
    np.cumsum([len(n) for n in CARDS], out=off[1:])
    blob = np.frombuffer("".join(CARDS).encode(), np.uint8)
    buf = np.full(len(want) + 8, 0xAB, np.uint8)
    status, n = ctypes.c_int32(-9), ctypes.c_int64(-9)

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    rc = l.pas_gas_annotation_render(2, 4, 4, ptr(c), ptr(off), ptr(blob), ctypes.byref(status),
                                     ptr(buf), len(want) - 1, ctypes.byref(n))
    assert (rc, status.value, n.value) == (_lib.PAS_ECAPACITY, OK, len(want))
    assert (buf == 0xAB).all()
    rc = l.pas_gas_annotation_render(2, 4, 4, ptr(c), ptr(off), ptr(blob), ctypes.byref(status),
                                     ptr(buf), len(want), ctypes.byref(n))
    assert rc == _lib.PAS_OK and buf[:len(want)].tobytes() == want
    assert (buf[len(want):] == 0xAB).all()  # nothing past the annotation
    # bad arguments
    assert l.pas_gas_annotation_render(-1, 4, 4, ptr(c), ptr(off), ptr(blob),
                                       ctypes.byref(status), ptr(buf), 8,
                                       ctypes.byref(n)) == _lib.PAS_EINVAL
    off_bad = off.copy()
    off_bad[2] = 1
    assert l.pas_gas_annotation_render(2, 4, 4, ptr(c), ptr(off_bad), ptr(blob),
                                       ctypes.byref(status), ptr(buf), 8,
                                       ctypes.byref(n)) == _lib.PAS_EINVAL
