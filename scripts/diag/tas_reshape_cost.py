#!/usr/bin/env python3
"""Diagnostic: a shape change of the resident TAS snapshot through pas_tas_snapshot_reshape
against the only route the snapshot offered before it (DESIGN.md "TAS reshape"; recorded, not
gated on a time).

Shapes: 100 000 x 64 and 1 000 000 x 64 (the deschedule configuration), about 70 % presence,
one column at scale 6.  Two changes:
  add_column   one empty column appended (a policy registered a metric)
  grow_nodes   the node count grown by one tier, max(64, N / 8) rounded up to 64 (TasCache's
               rule: a refresh listed a node first seen and no spare slot was left)
Reshape route: one pas_tas_snapshot_reshape call (allocation, the gather kernel, the
synchronize and the free of the old storage).  Old route: pas_tas_snapshot_set +
pas_tas_snapshot_set_scale of the full final content from host arrays, which includes the
host-link copy and two device-wide radix sorts.  Both routes end in a synchronize, so the host
clock around each call is the number: the median of --steps after --warmup, min and max beside
it.  The routes alternate within a step (each step first sets the start shape again, untimed)
and must leave the same snapshot (pas_tas_snapshot_get, checked once per change).

Also reported: the algorithmic bytes of the gather, read plus written and computed from the
shapes, over the reshape's call time, as a share of the 8.0 TB/s HBM peak.  The call time holds
more than the kernel (hipMalloc and hipFree of the whole storage), so the share is a floor.
One JSON line; fails without a GPU.

usage: tas_reshape_cost.py [--nodes 100000,1000000] [--metrics 64] [--steps 10] [--warmup 2]
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
from pas_amd.workload import pack_bits  # noqa: E402

HBM_PEAK = 8.0e12


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def order_row(n):
    return (n + 1023) // 1024 * 1024 + 1024


def gather_bytes(n0, m0, n1, m1, cnt_sum):
    """Bytes the gather reads (old vals and presence, the first cnt entries of sorted and of the
    three perm planes) and writes (every new array), narrow columns."""
    w0, w1, r1 = (n0 + 63) // 64, (n1 + 63) // 64, order_row(n1)
    read = m0 * n0 * 8 + m0 * w0 * 8 + cnt_sum * (8 + 3 * 4)
    written = m1 * n1 * 8 + m1 * w1 * 8 + m1 * r1 * (8 + 3 * 4) + m1 * (r1 // 32 + r1 // 1024) * 8
    return read + written


def padded(v, p_bool, scale, n1, m1):
    m0, n0 = v.shape
    v1 = np.zeros((m1, n1), np.int64)
    p1 = np.zeros((m1, n1), bool)
    s1 = np.full(m1, 3, np.int32)
    v1[:m0, :n0], p1[:m0, :n0], s1[:m0] = v, p_bool, scale
    return v1, pack_bits(p1), s1


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
        rng = np.random.default_rng(0x7A5 + N)
        v = rng.integers(0, 1_000_000, size=(M, N), dtype=np.int64)
        p_bool = rng.random((M, N)) < 0.7
        p = pack_bits(p_bool)
        scale = np.full(M, 3, np.int32)
        scale[1] = 6
        cnt_sum = int(p_bool.sum())
        grown = N + (max(64, N // 8) + 63) // 64 * 64
        res = {}
        for change, (n1, m1) in (("add_column", (N, M + 1)), ("grow_nodes", (grown, M))):
            final = padded(v, p_bool, scale, n1, m1)

            def start():
                gen[0] += 1
                ctx.tas_snapshot_set(gen[0], v, p, scale)

            def reshape():
                t0 = time.perf_counter()
                ctx.tas_snapshot_reshape(gen[0], gen[0] + 1, n1, m1)
                gen[0] += 1
                return (time.perf_counter() - t0) * 1e3

            def full_set():
                t0 = time.perf_counter()
                gen[0] += 1
                ctx.tas_snapshot_set(gen[0], final[0], final[1], final[2])
                return (time.perf_counter() - t0) * 1e3

            def same(x, y):  # values where present, presence, scales
                keep = np.unpackbits(x[2].view(np.uint8), axis=-1, bitorder="little")[:, :n1] != 0
                return (np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3]) and
                        np.array_equal(x[1][keep], y[1][keep]))

            start()
            reshape()
            got = ctx.tas_snapshot_get()
            start()
            full_set()
            assert same(got, ctx.tas_snapshot_get()), "the two routes leave different snapshots"
            del got
            r_ms, s_ms = [], []
            for _ in range(a.warmup + a.steps):
                start()
                r_ms.append(reshape())
                start()
                s_ms.append(full_set())
            r, s = stats(r_ms[a.warmup:]), stats(s_ms[a.warmup:])
            nbytes = gather_bytes(N, M, n1, m1, cnt_sum)
            res[change] = {"to": [n1, m1], "reshape": r, "full_set": s,
                           "speedup_median": s["median_ms"] / r["median_ms"],
                           "gather_bytes": nbytes,
                           "gather_share_of_hbm_peak":
                               nbytes / (r["median_ms"] * 1e-3) / HBM_PEAK,
                           "host_link_bytes_full_set": int(final[0].nbytes + final[1].nbytes),
                           "results_equal": True}
            note(f"N={N} {change}: {res[change]}")
        out["shapes"][str(N)] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
