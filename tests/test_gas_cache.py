"""GasCache (pas_amd/gas_cache.py): the reference cache's pod event path, handlePod's switch
over annotatedPods (node_resource_cache.go:305-400,493-538), and parse_annotation, the inverse
of annotation().  No GPU: the cache runs against a stub context that records its pas_gas_apply
calls and returns scripted statuses."""
import numpy as np
import pytest

import pas_amd
from pas_amd import _lib, gas_cache, snapshot
from pas_amd.gas_cache import (BAD_ARGS, ERR_INPUT, ERR_OVERFLOW, OK, POD_ADDED, POD_COMPLETED,
                               POD_DELETED, POD_UPDATED, SKIPPED, GasCache)

KINDS = ["gpu.intel.com/i915", "gpu.intel.com/memory.max"]
NODES = ["node-a", "node-b"]
CARDS = [["card0", "card1", "card2"], ["card0", "card1"]]
ADD, REMOVE = _lib.PAS_GAS_EV_ADD, _lib.PAS_GAS_EV_REMOVE


# ------------------------------------------------------------------ the C-ABI surface

def test_apply_symbols_present_and_bound():
    lib = pas_amd.LIB
    for name in ("pas_gas_apply", "pas_gas_apply_device"):
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["pas_gas_apply_device"][1]) == \
        len(_lib.SIGNATURES["pas_gas_apply"][1]) + 1  # + hip_stream
    assert (_lib.PAS_GAS_EV_ADD, _lib.PAS_GAS_EV_REMOVE) == (0, 1)
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "#define PAS_GAS_EV_ADD 0" in header and "#define PAS_GAS_EV_REMOVE 1" in header
    assert "#define PAS_ABI_VERSION 3" in header and "#define PAS_K_COUNT 10" in header
    assert callable(pas_amd.Context.gas_apply) and callable(pas_amd.Context.gas_apply_device)


# ------------------------------------------------------------------ parse_annotation

@pytest.mark.parametrize("word,i915,selection", [
    (0x80000000 | (3 << 24) | 0o210, [2, 1], None),        # card0,card1|card2
    (0x80000000 | (2 << 24) | 0o11, [0, 2], None),         # |card1,card1
    (0x80000000 | (1 << 24) | 2, [1], None),               # card2
    (0x80000000 | (15 << 24), [1, 0, 3], [2, 0, 0, 1]),    # an extended word's selection
])
def test_parse_annotation_round_trip(word, i915, selection):
    names = CARDS[0]
    text = snapshot.annotation(word, i915, names, selection)
    cpc, ranks = snapshot.parse_annotation(text, names)
    assert cpc == list(i915)
    want = selection if selection is not None else \
        [(word >> (3 * s)) & 7 for s in range((word >> 24) & 15)]
    assert ranks == want
    # and back: the same text from the parsed ranks
    assert snapshot.annotation(word, cpc, names, ranks) == text


def test_parse_annotation_split_cases():
    names = ["a", "b"]
    # strings.Split("", "|") is one empty segment: 0 cards
    assert snapshot.parse_annotation("", names) == ([0], [])
    # the "" inside "a,,b" is a name the label lacks: rank -1, and it counts
    assert snapshot.parse_annotation("a,,b", names) == ([3], [0, -1, 1])
    assert snapshot.parse_annotation("zzz|b,a", names) == ([1, 2], [-1, 1, 0])
    assert snapshot.parse_annotation("a||b,", names) == ([1, 0, 2], [0, 1, -1])
    assert snapshot.parse_annotation("|", names) == ([0, 0], [])
    assert snapshot.parse_annotation("b,b", []) == ([2], [-1, -1])


# ------------------------------------------------------------------ GasCache

class StubCtx:
    """Records gas_apply / gas_snapshot_set calls; statuses come from `script` (a list of
    lists, one per call; OK when it runs out)."""

    def __init__(self, script=()):
        self.calls, self.sets, self.script = [], [], list(script)

    def gas_apply(self, gen_from, gen_to, kinds, pods, nodes, req, mask, ncont, cpc, cards):
        self.calls.append(dict(gen_from=gen_from, gen_to=gen_to, kinds=list(kinds),
                               pods=list(pods), nodes=list(nodes), req=np.array(req),
                               mask=np.array(mask), ncont=list(ncont), cpc=np.array(cpc),
                               cards=np.array(cards)))
        st = self.script.pop(0) if self.script else [_lib.PAS_GAS_OK] * len(kinds)
        assert len(st) == len(kinds)
        return np.array(st, np.int32)

    def gas_snapshot_set(self, gen, n_cards, cap, used):
        self.sets.append((gen, np.array(n_cards), np.array(cap), np.array(used)))


def pod(name, annotation=None, node="node-a", containers=((1, 100),), phase="Running",
        deleting=False, ns="default"):
    meta = {"namespace": ns, "name": name}
    if annotation is not None:
        meta["annotations"] = {"gas-container-cards": annotation}
    if deleting:
        meta["deletionTimestamp"] = "2024-01-01T00:00:00Z"
    spec = {"nodeName": node, "containers": [
        {"name": f"c{i}", "resources": {"requests": {KINDS[0]: str(a), KINDS[1]: str(b)}}}
        for i, (a, b) in enumerate(containers)]}
    return {"metadata": meta, "spec": spec, "status": {"phase": phase}}


def cache(script=(), **kw):
    ctx = StubCtx(script)
    return ctx, GasCache(ctx, 100, NODES, CARDS, KINDS, **kw)


def test_is_completed_pod():
    # isCompletedPod (utils.go:52-71)
    assert not gas_cache.is_completed_pod(pod("p"))
    assert not gas_cache.is_completed_pod(pod("p", phase="Pending"))
    assert not gas_cache.is_completed_pod(pod("p", phase="Unknown"))
    assert gas_cache.is_completed_pod(pod("p", phase="Failed"))
    assert gas_cache.is_completed_pod(pod("p", phase="Succeeded"))
    assert gas_cache.is_completed_pod(pod("p", deleting=True))
    assert gas_cache.pod_key(pod("p", ns="ns1")) == "ns1&p"


def test_add_builds_the_event_from_the_annotation():
    ctx, gc = cache()
    p = pod("p", "card2,card0|card1,nope", node="node-a", containers=((2, 100), (2, 30)))
    gc.add_pod(p)
    gc.add_pod(pod("bare"))  # no annotation: waits for its update
    assert ctx.calls == []  # handlers only queue
    assert gc.flush() == [("default&p", POD_ADDED, OK)]
    (call,) = ctx.calls
    assert (call["gen_from"], call["gen_to"], gc.gen) == (100, 101, 101)
    assert call["kinds"] == [ADD] and call["nodes"] == [0] and call["pods"] == [0]
    assert call["ncont"] == [2]
    np.testing.assert_array_equal(call["req"], [[[2, 100], [2, 30]]])
    np.testing.assert_array_equal(call["mask"], [[3, 3]])
    np.testing.assert_array_equal(call["cpc"], [[2, 2]])
    np.testing.assert_array_equal(call["cards"], [[2, 0, 1, -1]])
    assert gc.annotated == {"default&p": "card2,card0|card1,nope"}


def test_add_then_update_of_the_same_key_is_applied_once():
    ctx, gc = cache()
    p = pod("p", "card0")
    gc.add_pod(p)
    gc.update_pod(None, p)
    out = gc.flush()
    assert out == [("default&p", POD_ADDED, OK), ("default&p", POD_UPDATED, SKIPPED)]
    assert len(ctx.calls) == 1 and ctx.calls[0]["kinds"] == [ADD]
    gc.update_pod(p, p)
    assert gc.flush() == [("default&p", POD_UPDATED, SKIPPED)]
    assert len(ctx.calls) == 1


@pytest.mark.parametrize("status,outcome", [(_lib.PAS_GAS_ERR_OVERFLOW, ERR_OVERFLOW),
                                            (_lib.PAS_GAS_ERR_INPUT, ERR_INPUT)])
def test_a_failed_add_is_retried_by_the_next_update(status, outcome):
    # annotatedPods changes only when the adjustment succeeded
    ctx, gc = cache(script=[[status]])
    p = pod("p", "card0")
    gc.add_pod(p)
    gc.update_pod(None, p)
    out = gc.flush()
    assert out == [("default&p", POD_ADDED, outcome), ("default&p", POD_UPDATED, OK)]
    assert [c["kinds"] for c in ctx.calls] == [[ADD], [ADD]]
    assert "default&p" in gc.annotated


def test_completed_releases_and_deleted_does_not():
    ctx, gc = cache()
    p = pod("p", "card1")
    gc.add_pod(p)
    gc.flush()
    done = pod("p", "card1", phase="Succeeded")
    gc.update_pod(p, done)
    assert gc.flush() == [("default&p", POD_COMPLETED, OK)]
    assert [c["kinds"] for c in ctx.calls] == [[ADD], [REMOVE]]
    np.testing.assert_array_equal(ctx.calls[1]["cards"], [[1]])
    assert gc.annotated == {}
    # completed again, then deleted: the annotation is already gone
    gc.update_pod(done, done)
    gc.delete_pod(done)
    assert gc.flush() == [("default&p", POD_COMPLETED, SKIPPED),
                          ("default&p", POD_DELETED, SKIPPED)]
    # a pod deleted while annotated: no usage is released (the item has no annotation)
    q = pod("q", "card0,card2")
    gc.add_pod(q)
    gc.delete_pod(q)
    assert gc.flush() == [("default&q", POD_ADDED, OK), ("default&q", POD_DELETED, OK)]
    assert [c["kinds"] for c in ctx.calls] == [[ADD], [REMOVE], [ADD]]
    assert gc.annotated == {}


def test_delete_quirk_one_container_versus_several():
    ctx, gc = cache()
    one = pod("one", "card0")
    two = pod("two", "card0|card1", containers=((1, 10), (1, 10)))
    gc.add_pod(one)
    gc.add_pod(two)
    gc.flush()
    n = len(ctx.calls)
    gc.delete_pod(one)
    gc.delete_pod(two)
    # "" is one segment: a no-op for one container (key forgotten), errBadArgs for two
    assert gc.flush() == [("default&one", POD_DELETED, OK), ("default&two", POD_DELETED, BAD_ARGS)]
    assert len(ctx.calls) == n
    assert gc.annotated == {"default&two": "card0|card1"}
    # the forgotten key is added again by its next update; the kept one is not
    gc.update_pod(None, one)
    gc.update_pod(None, two)
    assert gc.flush() == [("default&one", POD_UPDATED, OK), ("default&two", POD_UPDATED, SKIPPED)]


def test_bad_args_sends_nothing():
    ctx, gc = cache()
    gc.add_pod(pod("segs", "card0|card1"))                        # 2 segments, 1 container
    gc.add_pod(pod("fewer", "card0", containers=((1, 1), (1, 1))))  # 1 segment, 2 containers
    gc.add_pod(pod("nonode", "card0", node=""))
    out = gc.flush()
    assert [o[2] for o in out] == [BAD_ARGS, BAD_ARGS, BAD_ARGS]
    assert ctx.calls == [] and gc.annotated == {} and gc.gen == 100
    # a failed check leaves the key unannotated: the corrected update is applied
    gc.update_pod(None, pod("segs", "card0"))
    assert gc.flush() == [("default&segs", POD_UPDATED, OK)]
    assert len(ctx.calls) == 1


def test_note_bind_suppresses_the_echo():
    ctx, gc = cache()
    p = pod("p", "card0")
    gc.note_bind(p, "card0")
    gc.add_pod(p)
    gc.update_pod(None, p)
    assert [o[2] for o in gc.flush()] == [SKIPPED, SKIPPED]
    assert ctx.calls == []
    # its completion releases what the bind committed
    gc.update_pod(p, pod("p", "card0", deleting=True))
    assert gc.flush() == [("default&p", POD_COMPLETED, OK)]
    assert [c["kinds"] for c in ctx.calls] == [[REMOVE]]


def test_a_batch_is_cut_at_a_repeated_key():
    ctx, gc = cache()
    a, b, c = pod("a", "card0"), pod("b", "card1", node="node-b"), pod("c", "card2")
    gc.add_pod(a)
    gc.add_pod(b)
    gc.update_pod(a, pod("a", "card0", phase="Failed"))  # a again: closes the batch
    gc.add_pod(c)
    gc.update_pod(None, b)                              # b is annotated by then: skipped
    out = gc.flush()
    assert [o[2] for o in out] == [OK, OK, OK, OK, SKIPPED]
    assert [c_["kinds"] for c_ in ctx.calls] == [[ADD, ADD], [REMOVE, ADD]]
    assert [c_["nodes"] for c_ in ctx.calls] == [[0, 1], [0, 0]]
    assert [(c_["gen_from"], c_["gen_to"]) for c_ in ctx.calls] == [(100, 101), (101, 102)]
    assert set(gc.annotated) == {"default&b", "default&c"}


def test_batch_pads_containers_and_card_rows():
    ctx, gc = cache()
    gc.add_pod(pod("a", "card0"))
    gc.add_pod(pod("b", "card1,card0|card0", node="node-b", containers=((2, 8), (1, 4))))
    gc.flush()
    (call,) = ctx.calls
    assert call["ncont"] == [1, 2]
    np.testing.assert_array_equal(call["cpc"], [[1, 0], [2, 1]])
    np.testing.assert_array_equal(call["cards"], [[0, -1, -1], [1, 0, 0]])
    np.testing.assert_array_equal(call["req"], [[[1, 100], [0, 0]], [[2, 8], [1, 4]]])
    np.testing.assert_array_equal(call["mask"], [[3, 0], [3, 3]])


def test_rebuild_zeroes_the_usage_and_adds_every_annotated_pod():
    n_cards = np.array([3, 2], np.int32)
    cap = np.array([[4, 1000], [4, 1000]], np.int64)
    ctx, gc = cache(n_cards=n_cards, cap=cap)
    gc.note_bind(pod("stale", "card0"), "card0")
    pods = [pod("a", "card0"), pod("bare"), pod("b", "card1", node="node-b"),
            pod("done", "card2", phase="Succeeded")]
    out = gc.rebuild(pods)
    # the initial list delivers every pod through addPodToCache, completed ones included
    assert out == [("default&a", POD_ADDED, OK), ("default&b", POD_ADDED, OK),
                   ("default&done", POD_ADDED, OK)]
    ((gen, nc, cp, used),) = ctx.sets
    assert gen == 101 and used.shape == (2, 3, 2) and not used.any()
    np.testing.assert_array_equal(nc, n_cards)
    np.testing.assert_array_equal(cp, cap)
    (call,) = ctx.calls
    assert call["kinds"] == [ADD, ADD, ADD] and (call["gen_from"], call["gen_to"]) == (101, 102)
    assert set(gc.annotated) == {"default&a", "default&b", "default&done"}
