#!/usr/bin/env python3
"""Diagnostic: dead node slots dropped from the resident TAS snapshot through
pas_tas_snapshot_compact against the only route the snapshot offered before it (DESIGN.md
"TAS / GAS compaction"; recorded, not gated on a time).

Shapes: 100 000 x 64 and 1 000 000 x 64 (the deschedule configuration), about 70 % presence,
one column at scale 6, every column narrow.  Two drop sets: a random 10 % and a random 50 % of
the slots; the survivors move down in order, no spare slot is added.
Compact route: one pas_tas_snapshot_compact call (allocation, the map's upload, the five
kernels, the synchronize and the free of the old storage).  Old route: pas_tas_snapshot_get of
the whole content, the compaction of the columns on the host (numpy gather of the values, bit
unpack / gather / pack of the presence), pas_tas_snapshot_set + pas_tas_snapshot_set_scale,
which holds two host-link copies and two device-wide radix sorts.  Both routes end in a
synchronize, so the host clock around each is the number: the median of --steps after
--warmup, min and max beside it.  The routes alternate within a step (each step first sets the
start content again, untimed) and must leave the same snapshot (pas_tas_snapshot_get, checked
once per drop set).

Also reported: the algorithmic bytes of the compaction, read plus written and computed from
the shapes, over the call's time, as a share of the 8.0 TB/s HBM peak.  The call time holds
more than the kernels (hipMalloc and hipFree of the whole storage), so the share is a floor.
One JSON line; fails without a GPU.

usage: tas_compact_cost.py [--nodes 100000,1000000] [--metrics 64] [--steps 10] [--warmup 2]
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
from pas_amd.workload import pack_bits, unpack_bits  # noqa: E402

HBM_PEAK = 8.0e12


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def order_row(n):
    return (n + 1023) // 1024 * 1024 + 1024


def compact_bytes(n0, n1, m, cnt_sum):
    """Bytes the kernels read (the first cnt entries of the three perm planes twice, count and
    scatter, each with its 4-byte slot-map lookup; the ascending plane's sorted values; the map
    per column; the gathered values and, counted as a byte each, presence bits) and write (the
    slot map and every new array), narrow columns."""
    w1, r1 = (n1 + 63) // 64, order_row(n1)
    read = 2 * 3 * cnt_sum * (4 + 4) + cnt_sum * 8 + m * n1 * (4 + 8 + 1)
    written = n0 * 4 + n1 * 4 + m * n1 * 8 + m * w1 * 8 + m * r1 * (8 + 3 * 4) + \
        m * (r1 // 32 + r1 // 1024) * 8
    return read + written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="100000,1000000")
    ap.add_argument("--metrics", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ctx = pas_amd.Context(0)
    M = a.metrics
    out = {"metrics": M, "steps": a.steps, "warmup": a.warmup, "hbm_peak": HBM_PEAK, "shapes": {}}
    gen = [100]
    for N in [int(x) for x in a.nodes.split(",")]:
        rng = np.random.default_rng(0xC0A + N)
        v = rng.integers(0, 1_000_000, size=(M, N), dtype=np.int64)
        p_bool = rng.random((M, N)) < 0.7
        p = pack_bits(p_bool)
        scale = np.full(M, 3, np.int32)
        scale[1] = 6
        cnt_sum = int(p_bool.sum())
        res = {}
        for drop in (0.10, 0.50):
            src = np.sort(rng.permutation(N)[int(N * drop):]).astype(np.int32)
            n1 = len(src)

            def start():
                gen[0] += 1
                ctx.tas_snapshot_set(gen[0], v, p, scale)

            def compact():
                t0 = time.perf_counter()
                ctx.tas_snapshot_compact(gen[0], gen[0] + 1, src)
                gen[0] += 1
                return (time.perf_counter() - t0) * 1e3

            def host_route():
                t0 = time.perf_counter()
                _, vals, present, sc, _, _ = ctx.tas_snapshot_get()
                v1 = np.ascontiguousarray(vals[:, src])
                p1 = pack_bits(unpack_bits(present, N)[:, src])
                gen[0] += 1
                ctx.tas_snapshot_set(gen[0], v1, p1, sc)
                return (time.perf_counter() - t0) * 1e3

            def same(x, y):  # values where present, presence, scales
                keep = unpack_bits(x[2], n1)
                return (np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3]) and
                        np.array_equal(x[1][keep], y[1][keep]))

            start()
            compact()
            got = ctx.tas_snapshot_get()
            start()
            host_route()
            assert same(got, ctx.tas_snapshot_get()), "the two routes leave different snapshots"
            del got
            c_ms, h_ms = [], []
            for _ in range(a.warmup + a.steps):
                start()
                c_ms.append(compact())
                start()
                h_ms.append(host_route())
            c, h = stats(c_ms[a.warmup:]), stats(h_ms[a.warmup:])
            nbytes = compact_bytes(N, n1, M, cnt_sum)
            key = f"drop_{int(drop * 100)}"
            res[key] = {"to": [n1, M], "compact": c, "get_host_set": h,
                        "speedup_median": h["median_ms"] / c["median_ms"],
                        "compact_bytes": nbytes,
                        "compact_share_of_hbm_peak":
                            nbytes / (c["median_ms"] * 1e-3) / HBM_PEAK,
                        "host_link_bytes_get_host_set":
                            int(v.nbytes + p.nbytes + v.nbytes * n1 // N + p.nbytes * n1 // N),
                        "results_equal": True}
            note(f"N={N} {key}: {res[key]}")
        out["shapes"][str(N)] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
