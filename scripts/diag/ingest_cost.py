#!/usr/bin/env python3
"""Diagnostic: what one metric refresh costs from Quantity strings (DESIGN.md "Refresh from
Quantity literals", recorded, not gated on a time).

One metric over N nodes with values like "%d.%03d", refreshed again and again with new values.

  cache:   TasCache.write_metric(name, {node: quantity}) with the default (every value parsed
           on the host, three library calls per value, then the column update) against
           device_ingest=True (the strings packed into one blob, one batch parse, one
           pas_tas_snapshot_update_quantities).  Wall time of the whole call, packing included.
  split:   the new call on device-resident inputs, by stream-synchronised wall time of three
           calls on the same inputs: the parse alone (pas_quantities_to_wide_device), the order
           rebuild alone (pas_tas_snapshot_update_device of one column), and the whole
           pas_tas_snapshot_update_quantities_device; "summary + encode" is the whole minus the
           other two (it includes the call's one read-back and its synchronisations).

Median of --steps runs after --warmup (min - max beside it).  One JSON line.

usage: ingest_cost.py [--nodes 100000] [--steps 10] [--warmup 2] [--no-cache]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "platform-aware-scheduling_amd"))

import pas_amd  # noqa: E402
from pas_amd import snapshot as sn  # noqa: E402
from pas_amd.tas_cache import TasCache  # noqa: E402


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3),
            "max_ms": round(float(max(ms)), 3)}


def values(nodes, step):
    rng = np.random.default_rng(step)
    a = rng.integers(0, 100000, len(nodes))
    b = rng.integers(0, 1000, len(nodes))
    return {n: "%d.%03d" % (x, y) for n, x, y in zip(nodes, a.tolist(), b.tolist())}


def timed(fn, sync, steps, warmup):
    ms = []
    for i in range(warmup + steps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def cache_cost(n, steps, warmup, device_ingest):
    nodes = [f"node-{i}" for i in range(n)]
    ctx = pas_amd.Context(0)
    try:
        tc = TasCache.from_metrics(ctx, 1, {"m": values(nodes, 10**6)}, node_names=nodes,
                                   device_ingest=device_ingest)
        ms = []
        for i in range(warmup + steps):
            data = values(nodes, i)
            ctx.synchronize()
            t0 = time.perf_counter()
            tc.write_metric("m", data)
            ctx.synchronize()
            if i >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms)
    finally:
        ctx.close()


def split_cost(n, steps, warmup):
    nodes = [f"node-{i}" for i in range(n)]
    index = {name: i for i, name in enumerate(nodes)}
    ctx = pas_amd.Context(0)
    try:
        ctx.tas_snapshot_set(1, np.zeros((1, n), np.int64), np.zeros((1, (n + 63) // 64), np.uint64))
        col_off, entry_node, lit_off, blob = sn.pack_quantities({"m": values(nodes, 0)}, index,
                                                                ["m"])
        node_t = torch.from_numpy(entry_node).cuda()
        off_t = torch.from_numpy(lit_off).cuda()
        bytes_t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        whole = torch.zeros(n, dtype=torch.int64, device="cuda")
        nano = torch.zeros(n, dtype=torch.int32, device="cuda")
        dec = torch.zeros(n, dtype=torch.int32, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")
        v_t = torch.randint(0, 10**8, (1, n), dtype=torch.int64, device="cuda")
        p_t = torch.full((1, (n + 63) // 64), -1, dtype=torch.int64, device="cuda")
        gen = [1]

        def parse():
            ctx.quantities_to_wide_device(n, len(blob), off_t, bytes_t, whole, nano, dec, status)

        def rebuild():
            ctx.tas_snapshot_update_device(gen[0], gen[0] + 1, [0], v_t, p_t)
            gen[0] += 1

        def whole_call():
            ctx.tas_snapshot_update_quantities_device(gen[0], gen[0] + 1, [0], col_off, len(blob),
                                                      node_t, off_t, bytes_t)
            gen[0] += 1

        out = {"parse": timed(parse, ctx.synchronize, steps, warmup),
               "order_rebuild": timed(rebuild, ctx.synchronize, steps, warmup),
               "whole_call": timed(whole_call, ctx.synchronize, steps, warmup)}
        assert int(status.abs().sum()) == 0
        out["summary_encode_ms"] = round(out["whole_call"]["median_ms"] - out["parse"]["median_ms"]
                                         - out["order_rebuild"]["median_ms"], 3)
        out["bytes_per_literal"] = round(len(blob) / n, 2)
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cache", action="store_true", help="the split of the new call only")
    a = ap.parse_args()
    out = {"nodes": a.nodes, "steps": a.steps, "warmup": a.warmup}
    if not a.no_cache:
        out["cache_host_parse"] = cache_cost(a.nodes, a.steps, a.warmup, False)
        out["cache_device_ingest"] = cache_cost(a.nodes, a.steps, a.warmup, True)
    out["split"] = split_cost(a.nodes, a.steps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
