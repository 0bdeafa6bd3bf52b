"""GasCache with node events as strings (device_nodes=True) beside the default node path on two
contexts: a seeded trace of mixed node and pod items, and the cold start, with outcomes, the host
tables and the resident snapshot and card-name table equal after every flush."""
import numpy as np
import pytest

import pas_amd
from pas_amd.gas_cache import GasCache
from test_gas_cache_nodes import KINDS, node_obj, pod_obj

CARDS = [f"card{i}" for i in (0, 1, 10, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12)] + ["gpu-é", "a\x00b"]


@pytest.fixture(scope="module")
def other_ctx():
    c = pas_amd.Context(0)
    yield c
    c.close()


def resident(gc):
    ctx = gc.ctx
    off, blob = ctx.gas_card_names_get()
    noff, nblob = ctx.names_get()
    return (ctx.gas_snapshot_get()[1], *ctx.gas_snapshot_get_nodes()[1:], off.tolist(), blob,
            noff.tolist(), nblob)


def assert_equal_caches(a, b):
    assert a.node_names == b.node_names and a.max_cards == b.max_cards
    assert a.card_names == b.card_names and a.parked == b.parked
    assert np.array_equal(a.n_cards, b.n_cards) and np.array_equal(a.cap, b.cap)
    for x, y in zip(resident(a), resident(b)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    # the host rows are the device's
    _, n_cards, cap = a.ctx.gas_snapshot_get_nodes()
    assert np.array_equal(a.n_cards, n_cards) and np.array_equal(a.cap, cap)


def start(ctx, nodes, **kw):
    return GasCache.from_nodes(ctx, 1, nodes, KINDS, spare_nodes=2, device_events=True, **kw)


FIRST = [node_obj(f"node-{i}", CARDS[i:i + 3]) for i in range(6)]


def run_trace(caches, check):
    """About 200 items through both caches (device_nodes first), check(*caches) after every
    flush; what the trace reached and its length."""
    rng = np.random.default_rng(20261021)
    names = [f"node-{i}" for i in range(14)]  # 8 of them first seen: past the 2 spare slots
    pods, seen, n_items = {}, set(), 0
    reached = dict.fromkeys(["parked", "dropped", "more_nodes", "tier_16", "tier_64", "returned",
                             "first_seen"], False)
    deleted = set()
    for step in range(24):
        for _ in range(int(rng.integers(6, 12))):
            n_items += 1
            r = rng.random()
            name = names[int(rng.integers(0, 6 + min(step, 8)))]
            if r < 0.45:  # a label of 1 .. 7 cards (step 12: 10 cards, step 18: 20 cards)
                count = 10 if step == 12 else int(rng.integers(1, 8))
                cards = [CARDS[i] for i in rng.permutation(len(CARDS))[:count]]
                if step == 18:
                    cards = [f"wide{i}" for i in range(20)]
                if rng.random() < 0.3:
                    cards += cards[:2]  # duplicates: gpuCount above the card count
                reached["returned"] |= name in deleted
                reached["first_seen"] |= name not in caches[1].node_index
                deleted.discard(name)
                for gc in caches:
                    (gc.update_node if name in seen else gc.add_node)(
                        *([None] if name in seen else []), node_obj(name, cards))
                seen.add(name)
            elif r < 0.52:
                for gc in caches:
                    gc.update_node(None, node_obj(name, None))  # the label goes
            elif r < 0.6:
                deleted.add(name)
                for gc in caches:
                    gc.delete_node(node_obj(name, None))
            elif r < 0.85:
                cards = caches[1].card_names[caches[1].node_index[name]] \
                    if name in caches[1].node_index else []
                ann = ",".join(cards[:int(rng.integers(0, 3))]) or "nosuchcard"
                key = f"p{n_items}"
                pods[key] = pod_obj(key, name, [(1, int(rng.integers(1, 100)))], ann)
                for gc in caches:
                    gc.add_pod(pods[key])
            elif pods:
                key = sorted(pods)[int(rng.integers(0, len(pods)))]
                done = dict(pods.pop(key), status={"phase": "Succeeded"})
                for gc in caches:
                    gc.update_pod(None, done)
        got, want = (gc.flush() for gc in caches)
        assert got == want, step
        check(*caches)
        reached["parked"] |= any(caches[0].parked)
        reached["dropped"] |= any(r[2].startswith("dropped: ") for r in got)
        reached["more_nodes"] |= len(caches[0].node_names) > 8
        reached["tier_16"] |= caches[0].max_cards == 16
        reached["tier_64"] |= caches[0].max_cards == 64
    return reached, n_items


@pytest.mark.gpu
def test_seeded_trace_in_both_modes(ctx, other_ctx):
    caches = [start(ctx, FIRST, device_nodes=True), start(other_ctx, FIRST)]
    assert_equal_caches(*caches)
    reached, n_items = run_trace(caches, assert_equal_caches)
    assert 180 <= n_items <= 280
    assert all(reached.values()), reached  # the trace asserts on itself
    assert caches[0].ctx.gas_snapshot_get()[1].any(), "the pods left usage to move"


@pytest.mark.gpu
def test_cold_start_of_300_nodes(ctx, other_ctx):
    rng = np.random.default_rng(300)
    nodes = []
    for i in range(300):
        count = 12 if i == 177 else int(rng.integers(0, 9))  # one label past the 8 tier
        cards = [CARDS[j] for j in rng.permutation(len(CARDS))[:count]]
        nodes.append(node_obj(f"n{i:03d}", (cards + cards[:1]) if count else None))
    got = start(ctx, nodes, device_nodes=True)
    want = start(other_ctx, nodes)
    assert got.max_cards == 16 and len(got.node_names) == 302
    assert_equal_caches(got, want)
