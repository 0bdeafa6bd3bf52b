#!/usr/bin/env python3
"""Diagnostic: what pod events from annotation strings cost and save (DESIGN.md "Pod events
from annotation strings", recorded, not gated on a time).  name_table_cost.py's protocol: the
arms of a comparison alternate step by step, median of --steps runs after --warmup (min - max
beside it), a host clock around work that ends in a device synchronise.

  cache:     GasCache.rebuild of --pods pods over --nodes nodes (k = 8, 1-2 containers, 1-4
             cards per container), the default mode (the host splits, probes and ranks) against
             device_events=True, and requests(pod) of every pod timed alone: what stays on the
             host in both arms.
  resident:  on resident inputs of each --sizes events: pas_gas_annotations_resolve_device
             alone, pas_gas_apply_device alone on the same events already parsed, and the whole
             pas_gas_apply_annotations_device; the rest is the read-back and the fix-up.

One JSON line.

usage: annotation_cost.py [--pods 100000] [--nodes 10000] [--sizes 100000,1000000]
                          [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "platform-aware-scheduling_amd"))

import pas_amd  # noqa: E402
from pas_amd import _lib  # noqa: E402
from pas_amd import snapshot as sn  # noqa: E402
from pas_amd.gas_cache import GasCache  # noqa: E402

KINDS = ["gpu.intel.com/i915", "gpu.intel.com/memory.max"]
K = 8
CARDS = [f"card{c}" for c in range(K)]


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3),
            "max_ms": round(float(max(ms)), 3)}


def node_names(n):
    return ["node-%07d.zone-%d.example.net" % (i, i % 7) for i in range(n)]


def lists(rng, n_events):
    """Per event 1-2 containers of 1-4 cards: (n_containers [E], cards_per_container [E][2],
    ranks [E][8] (-1 past the list), annotation strings)."""
    ncont = rng.integers(1, 3, size=n_events).astype(np.int32)
    cpc = rng.integers(1, 5, size=(n_events, 2)).astype(np.int32)
    cpc[ncont == 1, 1] = 0
    ranks = rng.integers(0, K, size=(n_events, 8)).astype(np.int32)
    ranks[np.arange(8)[None, :] >= cpc.sum(axis=1)[:, None]] = -1
    anns = []
    for c, r in zip(cpc.tolist(), ranks.tolist()):
        first = ",".join(CARDS[x] for x in r[:c[0]])
        anns.append(first if not c[1] else first + "|" + ",".join(CARDS[x] for x in
                                                                  r[c[0]:c[0] + c[1]]))
    return ncont, cpc, ranks, anns


def cluster(n_nodes, n_pods, seed):
    """v1.Node and v1.Pod objects: every node lists 8 cards, every pod is bound and annotated."""
    rng = np.random.default_rng(seed)
    names = node_names(n_nodes)
    nodes = [{"metadata": {"name": name, "labels": {sn.GPU_LIST_LABEL: ".".join(CARDS)}},
              "status": {"allocatable": {KINDS[0]: str(4 * K), KINDS[1]: str(4000 * K)}}}
             for name in names]
    ncont, cpc, _, anns = lists(rng, n_pods)
    on = rng.integers(0, n_nodes, size=n_pods)
    pods = []
    for p in range(n_pods):
        containers = [{"name": f"c{c}", "resources": {"requests": {
            KINDS[0]: str(cpc[p, c]), KINDS[1]: str(100 * cpc[p, c])}}}
            for c in range(ncont[p])]
        pods.append({"metadata": {"namespace": "default", "name": "pod-%07d" % p,
                                  "annotations": {"gas-container-cards": anns[p]}},
                     "spec": {"nodeName": names[on[p]], "containers": containers},
                     "status": {"phase": "Running"}})
    return nodes, pods


def cache_cost(n_nodes, n_pods, steps, warmup):
    nodes, pods = cluster(n_nodes, n_pods, 11)
    arms = {"default": False, "device_events": True}
    ctxs = {k: pas_amd.Context(0) for k in arms}
    try:
        caches = {k: GasCache.from_nodes(ctxs[k], 1, nodes, KINDS, device_events=v)
                  for k, v in arms.items()}
        ms = {k: [] for k in arms}
        requests = []
        for i in range(warmup + steps):
            for k in arms:
                ctxs[k].synchronize()
                t0 = time.perf_counter()
                results = caches[k].rebuild(pods)
                ctxs[k].synchronize()
                if i >= warmup:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
                assert len(results) == n_pods and all(r[2] == "ok" for r in results)
            print("cache_rebuild step", i, file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            for pod in pods:
                caches["default"]._requests(pod)
            if i >= warmup:
                requests.append((time.perf_counter() - t0) * 1e3)
        used = {k: ctxs[k].gas_snapshot_get()[1] for k in arms}
        assert np.array_equal(used["default"], used["device_events"]) and used["default"].any()
        assert caches["default"].annotated == caches["device_events"].annotated
        out = {k: stats(v) for k, v in ms.items()}
        out["requests_alone"] = stats(requests)
        for k in arms:
            out[k]["requests_share"] = round(out["requests_alone"]["median_ms"]
                                             / out[k]["median_ms"], 3)
        return out
    finally:
        for c in ctxs.values():
            c.close()


def timed(fn, sync, steps, warmup):
    ms = []
    for i in range(warmup + steps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def resident_cost(n_events, n_nodes, steps, warmup):
    import torch
    rng = np.random.default_rng(n_events)
    n_pods, c, q = 4096, 2, len(KINDS)
    p_ncont, p_cpc, p_ranks, p_anns = lists(rng, n_pods)
    pods = rng.integers(0, n_pods, size=n_events).astype(np.int32)
    nodes = rng.integers(0, n_nodes, size=n_events).astype(np.int32)
    req = np.zeros((n_pods, c, q), np.int64)
    req[:, :, 0], req[:, :, 1] = p_cpc, 100 * p_cpc
    mask = np.where(p_cpc > 0, 3, 0).astype(np.int32)
    ann_off, ann_blob = sn.pack_names([p_anns[p] for p in pods.tolist()])
    ctx = pas_amd.Context(0)
    try:
        gen = [1]
        ctx.gas_snapshot_set(1, np.full(n_nodes, K, np.int32), np.full((n_nodes, q), 10**9),
                             np.zeros((n_nodes, K, q), np.int64))
        ctx.gas_card_names_set(n_nodes, K, *sn.pack_names(CARDS * n_nodes))
        t = {name: torch.from_numpy(a).cuda() for name, a in dict(
            kinds=np.zeros(n_events, np.int32), pods=pods, nodes=nodes, req=req, mask=mask,
            ncont=p_ncont, cpc=p_cpc[pods], cards=p_ranks[pods], off=ann_off).items()}
        blob_t = torch.frombuffer(bytearray(ann_blob), dtype=torch.uint8).cuda()
        st = [torch.full((n_events,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
        verdict, listed = (torch.zeros(n_events, dtype=torch.int32, device="cuda")
                           for _ in range(2))
        cpc_out = torch.zeros((n_events, c), dtype=torch.int32, device="cuda")
        cards_out = torch.zeros((n_events, 8), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # the inputs are resident before any arm runs

        def resolve():
            ctx.gas_annotations_resolve_device(n_events, t["pods"], t["nodes"], n_pods,
                                               t["ncont"], c, len(ann_blob), t["off"], blob_t, 8,
                                               verdict, listed, cpc_out, cards_out)

        def apply_parsed():
            ctx.gas_apply_device(gen[0], gen[0] + 1, n_events, t["kinds"], t["pods"], t["nodes"],
                                 n_pods, c, t["req"], t["mask"], t["ncont"], t["cpc"], t["cards"],
                                 8, st[0])
            gen[0] += 1

        def apply_strings():
            ctx.gas_apply_annotations_device(gen[0], gen[0] + 1, n_events, t["kinds"], t["pods"],
                                             t["nodes"], n_pods, c, t["req"], t["mask"],
                                             t["ncont"], len(ann_blob), t["off"], blob_t, st[1])
            gen[0] += 1

        arms = {"resolve_alone": resolve, "apply_device_on_parsed_arrays": apply_parsed,
                "apply_annotations_device": apply_strings}
        ms = {k: [] for k in arms}
        for i in range(warmup + steps):  # the arms alternate step by step
            for k, fn in arms.items():
                ms[k] += timed(fn, ctx.synchronize, 1, 0) if i >= warmup else \
                    timed(fn, ctx.synchronize, 0, 1)
        # the arms computed the same thing
        assert torch.equal(cpc_out, t["cpc"]) and torch.equal(cards_out, t["cards"])
        assert int((verdict != _lib.PAS_GAS_ANN_PENDING).sum()) == 0
        assert torch.equal(st[0], st[1]) and int((st[0] != _lib.PAS_GAS_OK).sum()) == 0
        assert ctx.gas_snapshot_get()[1].any()
        out = {k: stats(v) for k, v in ms.items()}
        out["annotation_bytes_per_event"] = round(len(ann_blob) / n_events, 2)
        out["readback_and_fixup_ms"] = round(
            out["apply_annotations_device"]["median_ms"] - out["resolve_alone"]["median_ms"]
            - out["apply_device_on_parsed_arrays"]["median_ms"], 3)
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    out = {"steps": a.steps, "warmup": a.warmup, "nodes": a.nodes, "pods": a.pods}
    if a.pods > 0:
        out["cache_rebuild"] = cache_cost(a.nodes, a.pods, a.steps, a.warmup)
        print("cache_rebuild done", file=sys.stderr, flush=True)
    for n in [int(x) for x in a.sizes.split(",") if x]:
        out["resident_%d" % n] = resident_cost(n, a.nodes, a.steps, a.warmup)
        print("resident_%d done" % n, file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
