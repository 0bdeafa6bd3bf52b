#!/usr/bin/env python3
"""Diagnostic: node events on the resident GAS snapshot through pas_gas_nodes_update_device
against the route the snapshot offered before it (DESIGN.md "Node events"; recorded, not gated
on a time).

C3 snapshot shape: 50 000 nodes x 8 cards x 3 kinds.  A batch of U updates, U = 1, 1 000 and
50 000 (every node's allocatable changed: a device-plugin rollout), each with new capacities
and a rotation of the row as its slot map.

Device route: pas_gas_nodes_update_device (key kernel, radix sort, update kernel) with every
input resident, --calls back-to-back calls between two stream events, per-call time = window /
calls; median of --steps windows after --warmup (min - max beside it).

Host route, what one changed node cost before: pas_gas_snapshot_get (the whole usage to the
host), the same change with numpy, pas_gas_snapshot_set (everything up again), timed together
with the host clock (both calls synchronize) and per part.

The first pas_gas_fit_device after each route is timed with stream events: both rebuild the
fit's derived data.  The two routes alternate within a step and must leave the same snapshot
(checked once per U).  One JSON line.

usage: gas_nodes_update.py [--nodes 50000] [--steps 20] [--warmup 3] [--calls 10]
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
from pas_amd import workload as wl  # noqa: E402

K, P = 8, 16


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    N = a.nodes
    ctx = pas_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream)
    snap = wl.make_gas_snapshot(N, seed=0xC3, k=K, var_cards=True)
    batch = wl.make_gas_batch(P, seed=0xC3)
    Q, C = snap.cap.shape[1], batch.req.shape[1]
    pod_dev = (dev(batch.req), dev(batch.req_mask), dev(batch.n_containers))
    res_t = torch.empty((P, N), dtype=torch.int32, device="cuda")
    gen = [10]
    ctx.gas_snapshot_set(gen[0], snap.n_cards, snap.cap, snap.used)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    def fit():
        ctx.gas_fit_device(gen[0], P, C, wl.I915, *pod_dev, res_t, stream=stream)

    out = {"shape": {"nodes": N, "cards": K, "kinds": Q, "pods": P, "steps": a.steps,
                     "warmup": a.warmup, "calls": a.calls},
           "snapshot_bytes": int(snap.used.nbytes), "updates": {}}
    rng = np.random.default_rng(0xC3)
    for U in (1, 1000, N):
        nodes = (np.arange(N) if U == N else rng.choice(N, size=U, replace=False)).astype(np.int32)
        ncs = snap.n_cards[nodes]
        caps = snap.cap[nodes] + 1
        src = np.tile(((np.arange(K) + 1) % K).astype(np.int32), (U, 1))
        upd_dev = (dev(nodes), dev(ncs), dev(caps), dev(src))
        st_t = torch.empty(U, dtype=torch.int32, device="cuda")

        def device_route():
            for _ in range(a.calls):
                ctx.gas_nodes_update_device(gen[0], gen[0] + 1, U, *upd_dev, st_t, stream=stream)
                gen[0] += 1

        def host_route():
            t0 = time.perf_counter()
            _, used = ctx.gas_snapshot_get()
            t1 = time.perf_counter()
            n_cards, cap = snap.n_cards.copy(), snap.cap.copy()  # (the binding's own tables)
            used[nodes] = used[nodes][:, src[0]]
            n_cards[nodes], cap[nodes] = ncs, caps
            t2 = time.perf_counter()
            gen[0] += 1
            ctx.gas_snapshot_set(gen[0], n_cards, cap, used)
            t3 = time.perf_counter()
            return [(t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3]

        # the two routes leave the same snapshot
        gen[0] += 1
        ctx.gas_snapshot_set(gen[0], snap.n_cards, snap.cap, snap.used)
        ctx.gas_nodes_update_device(gen[0], gen[0] + 1, U, *upd_dev, st_t, stream=stream)
        gen[0] += 1
        stream.synchronize()
        assert int((st_t != 0).sum()) == 0
        _, got_used = ctx.gas_snapshot_get()
        _, got_nc, got_cap = ctx.gas_snapshot_get_nodes()
        gen[0] += 1
        ctx.gas_snapshot_set(gen[0], snap.n_cards, snap.cap, snap.used)
        host_route()
        assert np.array_equal(ctx.gas_snapshot_get()[1], got_used)
        _, nc2, cap2 = ctx.gas_snapshot_get_nodes()
        assert np.array_equal(nc2, got_nc) and np.array_equal(cap2, got_cap)

        d_ms, d_fit, h_ms, h_fit = [], [], [], []
        for _ in range(a.warmup + a.steps):
            fit()  # derived data is current before either route
            d_ms.append(timed(device_route) / a.calls)
            d_fit.append(timed(fit))
            h_ms.append(host_route())
            h_fit.append(timed(fit))
        w = a.warmup
        h = np.array(h_ms[w:])
        out["updates"][str(U)] = {
            "nodes_update_device": stats(d_ms[w:]), "first_fit_after_device": stats(d_fit[w:]),
            "host_route_wall": stats(h[:, 0]), "host_get": stats(h[:, 1]),
            "host_numpy": stats(h[:, 2]), "host_set": stats(h[:, 3]),
            "first_fit_after_host": stats(h_fit[w:]), "results_equal": True}
        note(f"U={U}: {out['updates'][str(U)]}")
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
