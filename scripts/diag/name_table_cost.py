#!/usr/bin/env python3
"""Diagnostic: what the resident node-name table costs and saves (DESIGN.md "Resident name
table", recorded, not gated on a time).  ingest_cost.py's protocol: the arms of a comparison
alternate step by step, median of --steps runs after --warmup (min - max beside it).

  cache:   TasCache.write_metric of one metric over N nodes, end to end (packing included), the
           parent route (device_ingest=True) against device_names=True, in the steady state (no
           new node) and with 1 % first-seen nodes per refresh.
  lookup:  pas_names_resolve_device and the no-new-name pas_names_assign_device on resident
           inputs, next to the host loops they replace: a Python loop of pas_name_table_lookup
           calls (ctypes call overhead included: that is how a Python binding reaches it) and
           the Python dict probe TasCache._flush_literals runs per entry.
  table:   pas_names_set and pas_names_remap (dropping every 10th slot) of the whole table.

One JSON line.

usage: name_table_cost.py [--sizes 100000,1000000] [--steps 10] [--warmup 2]
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
from pas_amd import wire  # noqa: E402
from pas_amd.tas_cache import TasCache  # noqa: E402


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3),
            "max_ms": round(float(max(ms)), 3)}


def node_names(n):
    return ["node-%07d.zone-%d.example.net" % (i, i % 7) for i in range(n)]


def values(nodes, step):
    rng = np.random.default_rng(step)
    a = rng.integers(0, 100000, len(nodes))
    b = rng.integers(0, 1000, len(nodes))
    return {n: "%d.%03d" % (x, y) for n, x, y in zip(nodes, a.tolist(), b.tolist())}


def cache_cost(n, steps, warmup, new_share):
    """Both caches take the same refresh each step, the parent route first."""
    nodes = node_names(n)
    arms = {"device_ingest": False, "device_names": True}
    ctxs = {k: pas_amd.Context(0) for k in arms}
    try:
        caches = {k: TasCache.from_metrics(ctxs[k], 1, {"m": {}}, node_names=nodes,
                                           spare_metrics=1, device_ingest=True, device_names=v)
                  for k, v in arms.items()}
        ms = {k: [] for k in arms}
        n_new = int(n * new_share)
        for i in range(warmup + steps):
            live = nodes[:n - n_new] + ["late-%d-%07d.example.net" % (i, j) for j in range(n_new)]
            data = values(live, i)
            for k in arms:
                ctxs[k].synchronize()
                t0 = time.perf_counter()
                caches[k].write_metric("m", data)
                ctxs[k].synchronize()
                if i >= warmup:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        assert caches["device_ingest"].node_names == caches["device_names"].node_names
        return {k: stats(v) for k, v in ms.items()}
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
    return stats(ms)


def lookup_cost(n, steps, warmup):
    nodes = node_names(n)
    ctx = pas_amd.Context(0)
    host = wire.NameTable(nodes)
    try:
        off, blob = sn.pack_names(nodes)
        ctx.names_set(off, blob)
        out = {"bytes_per_name": round(len(blob) / n, 2)}
        perm = np.random.default_rng(n).permutation(n)
        entries = [nodes[i] for i in perm.tolist()]
        e_off, e_blob = sn.pack_names(entries)
        off_t = torch.from_numpy(e_off).cuda()
        bytes_t = torch.frombuffer(bytearray(e_blob), dtype=torch.uint8).cuda()
        slot_t = torch.zeros(n, dtype=torch.int32, device="cuda")
        index = {name: i for i, name in enumerate(nodes)}
        got = {}

        def resolve():
            ctx.names_resolve_device(n, len(e_blob), off_t, bytes_t, slot_t)

        def assign():
            ctx.names_assign_device(n, len(e_blob), off_t, bytes_t, slot_t)

        def c_loop():
            got["c"] = [host.lookup(name) for name in entries]

        def dict_loop():
            got["d"] = np.fromiter((index.get(name, -1) for name in entries), np.int32, n)

        def pack():
            sn.pack_names(entries)

        out["names_resolve_device"] = timed(resolve, ctx.synchronize, steps, warmup)
        assert np.array_equal(slot_t.cpu().numpy(), perm)
        out["names_assign_device_no_new"] = timed(assign, ctx.synchronize, steps, warmup)
        assert np.array_equal(slot_t.cpu().numpy(), perm)
        out["python_loop_of_pas_name_table_lookup"] = timed(c_loop, ctx.synchronize, steps, warmup)
        out["python_dict_probe_per_entry"] = timed(dict_loop, ctx.synchronize, steps, warmup)
        assert got["c"] == perm.tolist() and np.array_equal(got["d"], perm)
        out["pack_names"] = timed(pack, ctx.synchronize, steps, warmup)
        return out
    finally:
        host.close()
        ctx.close()


def table_cost(n, steps, warmup):
    nodes = node_names(n)
    ctx = pas_amd.Context(0)
    try:
        off, blob = sn.pack_names(nodes)
        src = np.array([i for i in range(n) if i % 10], np.int32)

        def set_():
            ctx.names_set(off, blob)

        def set_remap():
            ctx.names_set(off, blob)
            ctx.names_remap(src)

        out = {"names_set": timed(set_, ctx.synchronize, steps, warmup),
               "names_set_then_remap": timed(set_remap, ctx.synchronize, steps, warmup)}
        out["names_remap_ms"] = round(out["names_set_then_remap"]["median_ms"]
                                      - out["names_set"]["median_ms"], 3)
        n_slots, n_named, n_bytes = ctx.names_info()
        assert (n_slots, n_named) == (len(src), len(src))
        out["pool_bytes"] = n_bytes
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    out = {"steps": a.steps, "warmup": a.warmup}
    for n in [int(x) for x in a.sizes.split(",")]:
        out[str(n)] = {"cache_steady": cache_cost(n, a.steps, a.warmup, 0.0),
                       "cache_1pct_new": cache_cost(n, a.steps, a.warmup, 0.01),
                       "lookup": lookup_cost(n, a.steps, a.warmup)}
    out["table_%d" % n] = table_cost(n, a.steps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
