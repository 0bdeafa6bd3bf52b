"""The "gas-container-cards" grammar (csrc/annotation_fixed.h) on the CPU: the new symbols are
exported and bound, pas_gas_annotation_parse agrees with snapshot.parse_annotation / Python's
split on fixed and generated annotations, and the same header passes a stand-alone program under
ASan + UBSan.  The device runs the same routine per pod event (tests/test_gas_apply_annotations_
gpu.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib, snapshot
from pas_amd.context import gas_annotation_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "platform-aware-scheduling_amd", "csrc")

NEW_SYMBOLS = [
    "pas_gas_card_names_set", "pas_gas_card_names_update", "pas_gas_card_names_resize",
    "pas_gas_card_names_remap", "pas_gas_card_names_info", "pas_gas_card_names_get",
    "pas_gas_card_names_drop", "pas_gas_annotation_parse", "pas_gas_annotations_resolve",
    "pas_gas_annotations_resolve_device", "pas_gas_apply_annotations",
    "pas_gas_apply_annotations_device", "pas_gas_apply_annotations_names",
    "pas_gas_apply_annotations_names_device",
]


def test_new_symbols_present_and_bound():
    lib = pas_amd.LIB
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    sig = _lib.SIGNATURES
    for host in ("pas_gas_apply_annotations", "pas_gas_apply_annotations_names"):
        # the _device forms add the byte counts of their blobs and the stream
        blobs = 2 if host.endswith("_names") else 1
        assert len(sig[host + "_device"][1]) == len(sig[host][1]) + blobs + 1
    assert len(sig["pas_gas_annotations_resolve_device"][1]) == \
        len(sig["pas_gas_annotations_resolve"][1]) + 2
    assert (_lib.PAS_GAS_ERR_BAD_ARGS, _lib.PAS_GAS_ANN_PENDING) == (4, -1)
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "#define PAS_GAS_ERR_BAD_ARGS 4" in header
    assert "#define PAS_GAS_ANN_PENDING (-1)" in header
    assert "#define PAS_ABI_VERSION 3" in header  # additions only
    for method in ("gas_card_names_set", "gas_card_names_update", "gas_card_names_resize",
                   "gas_card_names_remap", "gas_card_names_info", "gas_card_names_get",
                   "gas_card_names_drop", "gas_annotations_resolve",
                   "gas_annotations_resolve_device", "gas_apply_annotations",
                   "gas_apply_annotations_device", "gas_apply_annotations_names",
                   "gas_apply_annotations_names_device"):
        assert callable(getattr(pas_amd.Context, method)), method


def reference(blob: bytes):
    """(segment counts, names) by Python's split on the bytes, as Go's strings.Split."""
    counts, names = [], []
    for segment in blob.split(b"|"):
        listed = segment.split(b",") if segment else []
        counts.append(len(listed))
        names.extend(listed)
    return counts, names


def check(blob: bytes, max_containers=None, cap=None):
    want_counts, want_names = reference(blob)
    segs, cpc, listed, spans = gas_annotation_parse(blob, max_containers, cap)
    assert segs == len(want_counts), blob
    assert listed == len(want_names), blob
    assert cpc == want_counts[:len(cpc)], blob
    assert len(cpc) == (segs if max_containers is None else min(max_containers, segs))
    assert len(spans) == (listed if cap is None else min(cap, listed))
    assert [blob[b:b + n] for b, n in spans] == want_names[:len(spans)], blob
    return want_counts, want_names


LONG = "x" * 300
FIXED = ["", "|", "||", ",", "a,", ",a", "a,,b", "a|", "|a", "card1,card10|card100",
         LONG, f"{LONG},{LONG}|{LONG}", b"a\x00b,\x00|\x00", "é,\xff|".encode() + b"\x80"]


@pytest.mark.parametrize("text", FIXED, ids=[repr(t)[:24] for t in FIXED])
def test_fixed_cases_match_split_and_parse_annotation(text):
    blob = text.encode() if isinstance(text, str) else text
    counts, names = check(blob)
    if isinstance(text, str):
        # the restatement the cache used so far: the same counts, and its ranks name the same
        # cards (every name its own card, in order of first appearance)
        table = list(dict.fromkeys(n.decode() for n in names))
        cpc, ranks = snapshot.parse_annotation(text, table)
        assert cpc == counts
        assert [table[r] for r in ranks] == [n.decode() for n in names]


def test_counts_by_hand():
    # strings.Split("", "|") is one empty segment; an empty segment lists no card; the empty
    # names of "a,,b", "a," and ",a" are names
    assert gas_annotation_parse("")[:3] == (1, [0], 0)
    assert gas_annotation_parse("|")[:3] == (2, [0, 0], 0)
    assert gas_annotation_parse("||")[:3] == (3, [0, 0, 0], 0)
    assert gas_annotation_parse(",") == (1, [2], 2, [(0, 0), (1, 0)])
    assert gas_annotation_parse("a,") == (1, [2], 2, [(0, 1), (2, 0)])
    assert gas_annotation_parse(",a") == (1, [2], 2, [(0, 0), (1, 1)])
    assert gas_annotation_parse("a,,b") == (1, [3], 3, [(0, 1), (2, 0), (3, 1)])
    assert gas_annotation_parse("a|")[:3] == (2, [1, 0], 1)
    assert gas_annotation_parse("|a") == (2, [0, 1], 1, [(1, 1)])
    assert gas_annotation_parse("card1,card10|card100") == \
        (2, [2, 1], 3, [(0, 5), (6, 6), (13, 7)])


def test_more_segments_than_max_containers_and_more_names_than_cap():
    blob = b"a,b|c|d,e,f||g"
    # the counts are always the full ones; the arrays stop at their sizes and not a word later
    assert gas_annotation_parse(blob, 2, 3) == (5, [2, 1], 7, [(0, 1), (2, 1), (4, 1)])
    assert gas_annotation_parse(blob, 0, 0) == (5, [], 7, [])
    lib = _lib.load()
    cpc = np.full(4, -7, np.int32)
    spans = np.full((5, 2), -7, np.int64)
    segs, listed = pas_amd.context.c_int64(), pas_amd.context.c_int64()
    rc = lib.pas_gas_annotation_parse(blob, len(blob), 2, pas_amd.context.byref(segs),
                                      cpc.ctypes.data, pas_amd.context.byref(listed),
                                      spans.ctypes.data, 3)
    assert rc == _lib.PAS_OK and (segs.value, listed.value) == (5, 7)
    assert cpc.tolist() == [2, 1, -7, -7]
    assert spans[3:].tolist() == [[-7, -7], [-7, -7]]
    # the span, not a terminator, ends the annotation
    assert gas_annotation_parse(b"a,b|c"[:3])[:3] == (1, [2], 2)
    # outputs are optional where their size is 0; a negative size is PAS_EINVAL
    assert lib.pas_gas_annotation_parse(b"a|b", 3, 0, None, None, None, None, 0) == _lib.PAS_OK
    assert lib.pas_gas_annotation_parse(b"a|b", -1, 0, None, None, None, None, 0) == \
        _lib.PAS_EINVAL
    assert lib.pas_gas_annotation_parse(b"a|b", 3, 1, None, None, None, None, 0) == \
        _lib.PAS_EINVAL


def test_random_strings():
    rng = np.random.default_rng(0xA770)
    alphabet = np.frombuffer(b"ab1,|\x00\xc3", np.uint8)
    shapes = set()
    for _ in range(5000):
        blob = alphabet[rng.integers(0, len(alphabet), size=int(rng.integers(0, 24)))].tobytes()
        counts, names = check(blob)
        check(blob, int(rng.integers(0, 5)), int(rng.integers(0, 9)))
        shapes.add((len(counts) > 1, len(names) > 0, b"" in names, 0 in counts))
    assert len(shapes) >= 8  # the generator reaches the grammar's corners


def test_standalone_program_under_sanitizers(tmp_path):
    """scripts/diag/annotation_parse_check.cpp: the header and the host entry point in a
    program of its own (nothing preloaded, nothing loaded into Python), built with ASan +
    UBSan; the fixed cases and 100 000 seeded random strings against a restated
    strings.Split."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer build of the host code"
    exe = tmp_path / "annotation_parse_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "scripts", "diag", "annotation_parse_check.cpp"),
                    os.path.join(CSRC, "gas_annotation.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.startswith("ok: ") and "100000 random strings" in run.stdout
