"""pas_gas_label_parse (csrc/label_fixed.h, the routines the device runs per node event) against
Go's reading of the cards label: len(strings.Split(s, ".")) pieces, and the distinct pieces in
sort.Strings order, counted up to PAS_GAS_MAX_CARDS + 1."""
import time

import pytest

from pas_amd import _lib
from pas_amd.context import gas_label_parse
from pas_amd.snapshot import go_sort_strings

STOP = _lib.PAS_GAS_MAX_CARDS + 1


def reference(label: bytes):
    pieces = label.split(b".")
    return len(pieces), sorted(set(pieces))  # bytes sort bytewise, a prefix first


def parsed(label: bytes):
    n_pieces, n_cards, spans = gas_label_parse(label)
    assert len(spans) == n_cards
    return n_pieces, n_cards, [label[b:b + l] for b, l in spans]


LABELS = [
    b"", b".", b"a..b", b"card1.card10.card2", b"card2.card10.card1", b"..", b"a.", b".a",
    b"card0.card1.card0.card1.card0",                       # duplicates
    b"card.card1.car.card10.c",                             # prefix chains
    b"x" * 70 + b"a." + b"x" * 70 + b"c." + b"x" * 70 + b"b",  # differ in the last byte, past 64
    b"a\x00b.a\x00a.a.\x00.a\x00",                          # byte 0 is an ordinary byte
    b"\xff.\x80.\x7f.a\xc3\xa9.a\xc3.\xfe\xff",              # bytes >= 0x80 sort above ASCII
    "é.e.z".encode(),
]


@pytest.mark.parametrize("label", LABELS)
def test_against_go_split_and_sort(label):
    n_pieces, cards = reference(label)
    assert parsed(label) == (n_pieces, len(cards), cards)


def test_str_labels_match_go_sort_strings():
    for s in ["", ".", "a..b", "card1.card10.card2", "b.a.b", "é.e"]:
        want = go_sort_strings(set(s.split(".")))
        n_pieces, n_cards, names = parsed(s.encode())
        assert (n_pieces, [n.decode() for n in names]) == (len(s.split(".")), want)


def test_documented_order():
    assert parsed(b"card2.card10..card1")[2] == [b"", b"card1", b"card10", b"card2"]


@pytest.mark.parametrize("distinct", [64, 65, 200])
def test_the_count_stops_at_65(distinct):
    label = b".".join(b"gpu%03d" % (distinct - i) for i in range(distinct))
    n_pieces, n_cards, names = parsed(label)
    assert n_pieces == distinct and n_cards == min(distinct, STOP)
    assert names == sorted(label.split(b"."))[:STOP]  # the 65 lowest, in rank order


def test_ten_thousand_copies_of_one_name():
    assert parsed(b".".join([b"card7"] * 10000)) == (10000, 1, [b"card7"])


def test_hostile_label_costs_65_passes_not_its_square():
    label = b".".join(b"%05d" % i for i in range(20000))  # 20 000 distinct names, 120 kB
    t0 = time.perf_counter()
    n_pieces, n_cards, names = parsed(label)
    assert (n_pieces, n_cards) == (20000, STOP) and names == [b"%05d" % i for i in range(STOP)]
    assert time.perf_counter() - t0 < 5.0  # 65 passes over 120 kB; the square would be minutes


def test_cap_and_arguments():
    assert gas_label_parse(b"b.a.c", cap=2) == (3, 3, [(2, 1), (0, 1)])
    assert gas_label_parse(b"b.a.c", cap=0) == (3, 3, [])
    lib = _lib.load()
    assert lib.pas_gas_label_parse(b"a.b", 3, None, None, None, 0) == _lib.PAS_OK
    assert lib.pas_gas_label_parse(b"a.b", -1, None, None, None, 0) == _lib.PAS_EINVAL
    assert lib.pas_gas_label_parse(b"a.b", 3, None, None, None, 1) == _lib.PAS_EINVAL
    assert lib.pas_gas_label_parse(None, 0, None, None, None, 0) == _lib.PAS_OK
