#!/usr/bin/env python3
"""Diagnostic: what the batch-of-requests verbs cost against the routes they replace
(DESIGN.md "Batches of requests in request terms"; recorded, not gated on a ratio).

N = 100 000 nodes; R = 1, 16 and 256 requests of 1 000 nodes each.

  prioritize  pas_tas_prioritize_requests (one call) against a loop of R
              pas_tas_prioritize_request calls (that entry point is unchanged: the yardstick)
  gas filter  pas_gas_fit_requests (one call) against one pas_gas_fit of the R pods over all N
              nodes followed by the host gather of each request's verdict bits
  cap         one request of S = 2 048 nodes, the longest one workgroup sorts in LDS, through
              both prioritize routes

All calls are the synchronous host forms through the Python binding, so a cost is wall time
per call.  The two arms of a comparison alternate; a sample is `inner` back-to-back calls (so
that it lasts tens of milliseconds), repeated --repeats times: median, min - max.  The outputs
of the two arms are compared at the timed sizes first.  One JSON line; "r1_ok" says whether at
R = 1 the batch form lies within the loop's own min - max spread or is faster.

usage: request_batch_cost.py [--nodes 100000] [--req 1000] [--repeats 7] [--warmup 2]
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
from pas_amd import workload as wl  # noqa: E402
from pas_amd.context import RULE_DTYPE, w64  # noqa: E402


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4),
            "max_ms": round(float(max(ms)), 4)}


def compare(arm_a, arm_b, repeats, warmup, target_ms=40.0):
    """Per-call milliseconds of two arms, alternated; inner calls sized from a first call."""
    out = []
    inner = []
    for arm in (arm_a, arm_b):
        for _ in range(warmup):
            arm()
        t = time.perf_counter()
        arm()
        inner.append(max(1, min(500, int(target_ms / max((time.perf_counter() - t) * 1e3, 1e-3)))))
        out.append([])
    for _ in range(repeats):
        for i, arm in enumerate((arm_a, arm_b)):
            t = time.perf_counter()
            for _ in range(inner[i]):
                arm()
            out[i].append((time.perf_counter() - t) * 1e3 / inner[i])
    return stats(out[0]), stats(out[1])


def pack_rows(bits_per_request, ld):
    rows = np.zeros((len(bits_per_request), ld), np.uint64)
    for r, b in enumerate(bits_per_request):
        by = np.packbits(b, bitorder="little")
        rows[r].view(np.uint8)[: len(by)] = by
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--metrics", type=int, default=8)
    ap.add_argument("--req", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.repeats >= 5
    rng = np.random.default_rng(0x5EED)
    ctx = pas_amd.Context(0)
    snap = wl.make_tas_snapshot(a.nodes, a.metrics, seed=0xD1)
    ctx.tas_snapshot_set(1, snap.v_milli, snap.present)
    gs = wl.make_gas_snapshot(a.nodes, seed=0xD2)
    ctx.gas_snapshot_set(2, gs.n_cards, gs.cap, gs.used)
    result = {"nodes": a.nodes, "req_nodes": a.req, "repeats": a.repeats, "prioritize": {},
              "gas_filter": {}}

    def requests(R, n):
        reqs = [rng.permutation(a.nodes)[:n].astype(np.int32) for _ in range(R)]
        off = (np.arange(R + 1) * n).astype(np.int32)
        return reqs, off, np.concatenate(reqs)

    def prio_arms(R, n):
        reqs, off, node = requests(R, n)
        prio = np.zeros(R, RULE_DTYPE)
        prio["metric"] = rng.integers(0, a.metrics, R)
        prio["op"] = rng.integers(0, 2, R)

        def batch():
            return ctx.tas_prioritize_requests(1, off, prio, node)

        def loop():
            return [ctx.tas_prioritize_request(1, prio[r], reqs[r]) for r in range(R)]

        pos, lens = batch()
        for r, one in enumerate(loop()):
            assert lens[r] == len(one) and np.array_equal(pos[off[r]: off[r] + lens[r]], one)
        return batch, loop

    for R in (1, 16, 256):
        b, l = compare(*prio_arms(R, a.req), a.repeats, a.warmup)
        result["prioritize"][f"R{R}"] = {"batch": b, "loop": l}
    b, l = compare(*prio_arms(1, 2048), a.repeats, a.warmup)
    result["cap"] = {"S": 2048, "R1": {"batch": b, "loop": l}}
    b, l = compare(*prio_arms(16, 2048), a.repeats, a.warmup)
    result["cap"]["R16"] = {"batch": b, "loop": l}

    for R in (1, 16, 256):
        reqs, off, node = requests(R, a.req)
        gb = wl.make_gas_batch(R, seed=0xD3 + R)
        ld = w64(a.req)

        def batch():
            return ctx.gas_fit_requests(2, off, node, gb.req, gb.req_mask, gb.n_containers,
                                        wl.I915)

        def all_nodes():
            res = ctx.gas_fit(2, gb.req, gb.req_mask, gb.n_containers, wl.I915)
            return pack_rows([(res[r, reqs[r]] >> 31).astype(np.uint8) for r in range(R)], ld)

        assert np.array_equal(batch(), all_nodes())
        b, l = compare(batch, all_nodes, a.repeats, a.warmup)
        result["gas_filter"][f"R{R}"] = {"batch": b, "all_nodes_then_gather": l}

    result["r1_ok"] = {
        "prioritize": result["prioritize"]["R1"]["batch"]["median_ms"]
        <= result["prioritize"]["R1"]["loop"]["max_ms"],
        "gas_filter": result["gas_filter"]["R1"]["batch"]["median_ms"]
        <= result["gas_filter"]["R1"]["all_nodes_then_gather"]["max_ms"],
    }
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
