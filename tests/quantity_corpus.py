"""Quantity literals for the fixed-width parser's tests, and what the host parser
(csrc/quantity.cpp, pinned by tests/golden/quantity_literals.json) makes of each.

The yardstick is always the host functions pas_quantity_to_wide / pas_quantity_decimals /
pas_quantity_to_scaled; the three literals whose exponents the host parser cannot take (signed
overflow near +-2^31) are pinned by hand in HUGE_EXPONENT."""
import functools
import json
import os
import random
import re
from ctypes import byref, c_int32, c_int64, c_uint32

from pas_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
OK, EINVAL, ENOTEXACT = _lib.PAS_OK, _lib.PAS_EINVAL, _lib.PAS_ENOTEXACT
INT64_MAX = 2**63 - 1

# (literal, (status, whole, nano, decimals)) checked against the host parser's documented steps
QUIRKS = [
    ("+", (OK, 0, 0, 0)), ("-", (OK, 0, 0, 0)), ("0", (OK, 0, 0, 0)), ("-0", (OK, 0, 0, 0)),
    ("0000000000000000001", (OK, 1, 0, 0)),
    ("10000000000000000000", (OK, INT64_MAX, 0, 0)),
    ("-10000000000000000000", (OK, -INT64_MAX, 0, 0)),
    ("1e19", (ENOTEXACT, 0, 0, 0)), ("-1e19", (ENOTEXACT, 0, 0, 0)),
    ("0.0000000000000000000001", (OK, 0, 1, 9)), ("1e-10", (OK, 0, 1, 9)), ("0.5n", (OK, 0, 1, 9)),
    ("-0.0000000000000000000001", (OK, -1, 999999999, 9)),
    ("-0.5", (OK, -1, 500000000, 1)),
    ("1.5Ki", (OK, 1536, 0, 0)), ("0.1Ki", (OK, 102, 400000000, 1)),
    ("8Ei", (OK, INT64_MAX, 0, 0)), ("1Pi", (OK, 2**50, 0, 0)),
    ("1K", (EINVAL,)), ("1i", (EINVAL,)), ("1Ki1", (EINVAL,)), ("5e", (EINVAL,)),
    ("5E+", (EINVAL,)), (" 1", (EINVAL,)), ("1 ", (EINVAL,)),
    ("1.", (OK, 1, 0, 0)), ("1.e3", (OK, 1000, 0, 0)), (".5", (OK, 0, 500000000, 1)),
    ("1e+3", (OK, 1000, 0, 0)),
    ("1e9223372036854775808", (EINVAL,)),
    # a dropped fraction under a binary suffix that comes out exact: 2^-69 * 2^60 * 1e9 = 5^9 n
    ("0." + "%069d" % (5**69) + "Ei", (OK, 0, 5**9, 9)),
    # ... and one digit more, far past the kept digits, that rounds it up
    ("0." + "%069d" % (5**69) + "0" * 40 + "1Ei", (OK, 0, 5**9 + 1, 9)),
]
# the host parser overflows int32 on these (UB): the documented steps, by hand
HUGE_EXPONENT = [
    ("1e2147483647", (ENOTEXACT, 0, 0, 0, -1)),
    ("1e-2147483647", (OK, 0, 1, 9, 9)),
    ("1e4294967296", (OK, 1, 0, 0, 9)),  # int32(parsed) truncates to 0
]
# bytes the host functions cannot be given (they take C strings)
NUL_INSIDE = [b"1\x002", b"\x00", b"12\x00", b"1.5\x00Ki"]


def golden_literals():
    with open(os.path.join(HERE, "golden", "quantity_literals.json")) as f:
        return [e["literal"] for e in json.load(f)["literals"]]


def generate(n, seed=20261020):
    """The corpus generator: n non-empty literals."""
    rng = random.Random(seed)
    digits = "0123456789"
    out = []
    while len(out) < n:
        s = rng.choice(["", "", "", "+", "-", "-"])
        s += "0" * rng.choice([0, 0, 0, 1, 3])
        k = rng.choice([0, 1, 1, 2, 3, 5, 8, 12, 17, 18, 19, 20, 25])
        if k:
            s += rng.choice(digits[1:]) + "".join(rng.choice(digits) for _ in range(k - 1))
        if rng.random() < 0.5:
            k = rng.choice([0, 1, 2, 3, 4, 6, 9, 10, 12, 20, 25])
            s += "." + "".join(rng.choice(digits) for _ in range(k))
        r = rng.random()
        if r < 0.6:
            s += rng.choice(["", "", "", "n", "u", "m", "k", "M", "G", "T", "P", "E", "Ki", "Mi",
                             "Gi", "Ti", "Pi", "Ei"])
        elif r < 0.9:
            s += rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randint(0, 40))
        if rng.random() < 0.06:
            at = rng.randint(0, len(s))
            s = s[:at] + rng.choice(" Kixe.-+,_9") + s[at:]
        if s:
            out.append(s)
    return out


def host_comparable(lit):
    """The host parser is the yardstick only for |exponent| <= 1000."""
    m = re.search(r"[eE][+-]?(\d+)$", lit)
    return m is None or int(m.group(1)) <= 1000


def host_reference(lit):
    """(status, whole, nano, decimals, fit) from the host functions: whole / nano 0 unless
    PAS_OK, decimals 0 for PAS_EINVAL, fit the largest places at which to_scaled succeeds."""
    lib = _lib.load()
    q = lit.encode()
    whole, nano, dec, v = c_int64(), c_uint32(), c_int32(), c_int64()
    status = lib.pas_quantity_to_wide(q, byref(whole), byref(nano))
    if status == EINVAL:
        return (EINVAL, 0, 0, 0, -1)
    assert lib.pas_quantity_decimals(q, byref(dec)) == OK
    fit = max([s for s in range(10) if lib.pas_quantity_to_scaled(q, s, byref(v)) == OK],
              default=-1)
    if status != OK:
        return (status, 0, 0, dec.value, fit)
    return (OK, whole.value, nano.value, dec.value, fit)


@functools.lru_cache(maxsize=None)
def corpus(n=20000):
    """((literal, ...), (reference, ...)) of the generated corpus, computed once."""
    lits = tuple(l for l in generate(n) if host_comparable(l))
    return lits, tuple(host_reference(l) for l in lits)


def pack(literals):
    """(lit_off int64 [n + 1] as a list, blob bytes) of literals given as str or bytes."""
    off, parts = [0], []
    for l in literals:
        b = l.encode() if isinstance(l, str) else bytes(l)
        parts.append(b)
        off.append(off[-1] + len(b))
    return off, b"".join(parts)
