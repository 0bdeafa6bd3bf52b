"""pas_quantity_as_int64_fixed (the AsInt64 field of csrc/quantity_fixed.h, the routine the
device runs per allocatable literal) against pas_quantity_as_int64 (csrc/quantity.cpp): equal
values on the generated corpus, the golden literals and the documented zeros, equal statuses for
what ParseQuantity rejects, and a byte 0 inside the span."""
import json
import os
from ctypes import byref, c_int64

import pytest

import quantity_corpus as qc
from pas_amd import _lib
from pas_amd.context import quantity_as_int64_fixed

HERE = os.path.dirname(os.path.abspath(__file__))
OK, EINVAL, ENOTEXACT = _lib.PAS_OK, _lib.PAS_EINVAL, _lib.PAS_ENOTEXACT


def host(lit):
    """(status, value) of pas_quantity_as_int64 (value 0 when it does not parse)."""
    out = c_int64()
    rc = _lib.load().pas_quantity_as_int64(lit.encode(), byref(out))
    return rc, out.value if rc == OK else 0


def test_equals_the_host_parser_on_the_corpus():
    lits, _ = qc.corpus()
    assert len(lits) > 15000
    seen = {"zero": 0, "value": 0, "invalid": 0}
    for lit in lits:
        rc, want = host(lit)
        got_rc, got = quantity_as_int64_fixed(lit)
        assert got == want, lit
        assert (got_rc == EINVAL) == (rc == EINVAL), lit
        seen["invalid" if rc == EINVAL else "value" if want else "zero"] += 1
    assert min(seen.values()) > 500, seen  # the corpus reaches every outcome


def test_golden_as_int64_entries():
    with open(os.path.join(HERE, "golden", "quantity_literals.json")) as f:
        entries = [e for e in json.load(f)["literals"] if "as_int64" in e]
    assert len(entries) > 10
    for e in entries:
        assert quantity_as_int64_fixed(e["literal"]) == (OK, int(e["as_int64"])), e
        assert host(e["literal"]) == (OK, int(e["as_int64"])), e


@pytest.mark.parametrize("lit,want", [
    ("1000m", 0), ("10.0", 0), ("1Pi", 0), ("1234567890123456789", 0), ("1.5Ki", 0),  # the zeros
    ("9223372036854775807", 0),  # 19 digits: an inf.Dec
    ("922337203685477580", 922337203685477580), ("-922337203685477580", -922337203685477580),
    ("1e18", 10**18), ("9e18", 9 * 10**18), ("-9e18", -9 * 10**18), ("92e17", 92 * 10**17),
    ("93e17", 0),  # past 2^63 - 1
    ("1e19", 0), ("-1e19", 0), ("1.5e3", 1500), ("1.5e1", 15), ("1.5e0", 0), ("12k", 12000),
    ("4Ki", 4096), ("8Gi", 8 << 30), ("-3Mi", -(3 << 20)), ("16384Pi", 0), ("0", 0), ("-0", 0),
    ("+7", 7), ("0e100", 0), ("007", 7), (".5", 0), ("5.", 5), ("1E", 10**18), ("10E", 0),
])
def test_documented_values(lit, want):
    rc, value = host(lit)
    assert (rc, value) == (OK, want), "the host parser itself"
    got_rc, got = quantity_as_int64_fixed(lit)
    assert got == want and got_rc in (OK, ENOTEXACT)
    assert (got_rc == ENOTEXACT) == (lit in ("1e19", "-1e19", "93e17", "10E"))


def test_statuses_of_unparsable_spans():
    for lit in ["", "1K", "1i", "1Ki1", "5e", "5E+", " 1", "1 ", "abc", "1e9223372036854775808",
                "--1", "1..2", "1,5"]:
        rc = _lib.load().pas_quantity_as_int64(lit.encode(), byref(c_int64())) if lit else EINVAL
        assert rc == EINVAL, lit
        assert quantity_as_int64_fixed(lit) == (EINVAL, 0), lit
    for raw in qc.NUL_INSIDE:  # a byte 0 inside the span ends no literal: it is a bad byte
        assert quantity_as_int64_fixed(raw) == (EINVAL, 0), raw
    # the span is what counts, not a terminator
    assert _lib.load().pas_quantity_as_int64_fixed(b"12k34", 3, byref(c_int64())) == OK
    out = c_int64()
    _lib.load().pas_quantity_as_int64_fixed(b"12k34", 3, byref(out))
    assert out.value == 12000
    assert _lib.load().pas_quantity_as_int64_fixed(b"12k", 3, None) == OK  # out may be NULL
