#!/usr/bin/env python3
"""Diagnostic: the cold-start rebuild of the GAS usage through pas_gas_apply_device
(DESIGN.md "Pod events", recorded, not gated on a time).

C3 cluster shape: 50 000 nodes x 8 cards x 4 kinds, zero usage, then 1 000 000 ADD events of
1 to 2 containers with cards_ld 8 (every running pod's annotation as one batch).

Device path: pas_gas_apply_device end to end (key kernel, radix sort, commit kernel) between
two stream events; median of --steps calls after --warmup (min - max beside it), the zero
snapshot uploaded again outside the timed region before each call.  The kernels' shares come
from a kernel trace of this script in a run of its own (--steps small, --no-host).

What the snapshot offered for the same job before the event path: the usage computed on the
host (numpy, np.add.at over the listed cards; no overflow or input checks) and uploaded whole
with pas_gas_snapshot_set.  Both parts are timed with the host clock (the upload call
synchronizes) and reported separately.  The two routes must leave the same usage (checked).
One JSON line.

usage: gas_apply_rebuild.py [--nodes 50000] [--events 1000000] [--steps 20] [--warmup 3]
                            [--no-host]
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
from pas_amd import _lib  # noqa: E402

K, Q, C, LD = 8, 4, 2, 8


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def make_events(n_nodes, n_events, n_pods, seed):
    rng = np.random.default_rng(seed)
    ncont = rng.integers(1, C + 1, size=n_pods).astype(np.int32)
    req = np.zeros((n_pods, C, Q), np.int64)
    req[:, :, 0] = rng.integers(1, 5, size=(n_pods, C))
    req[:, :, 1] = rng.integers(0, 1000, size=(n_pods, C))
    req[:, :, 2] = rng.integers(0, 1 << 30, size=(n_pods, C))
    req[:, :, 3] = rng.integers(0, 100, size=(n_pods, C))
    mask = np.full((n_pods, C), (1 << Q) - 1, np.uint32)
    pods = rng.integers(0, n_pods, size=n_events).astype(np.int32)
    nodes = rng.integers(0, n_nodes, size=n_events).astype(np.int32)
    cpc = rng.integers(1, LD // C + 1, size=(n_events, C)).astype(np.int32)
    cpc[ncont[pods] < 2, 1] = 0
    cards = rng.integers(0, K, size=(n_events, LD)).astype(np.int32)
    return req, mask, ncont, pods, nodes, cpc, cards


def host_rebuild(n_nodes, req, mask, ncont, pods, nodes, cpc, cards):
    """used [N][K][Q] of the ADD batch on zero usage, on the host."""
    used = np.zeros((n_nodes, K, Q), np.int64)
    off = np.zeros(len(pods), np.int64)
    slot = np.arange(LD)[None, :]
    for c in range(C):
        n = np.where(ncont[pods] > c, cpc[:, c], 0).astype(np.int64)
        share = req[pods, c] // np.maximum(n, 1)[:, None]          # divide(numCards), >= 0
        share *= ((mask[pods, c][:, None] >> np.arange(Q)) & 1).astype(np.int64)
        listed = (slot >= off[:, None]) & (slot < (off + n)[:, None])  # [E][LD]
        e, j = np.nonzero(listed)
        np.add.at(used, (nodes[e], cards[e, j]), share[e])
        off += n
    return used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--pods", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    N, E, P = a.nodes, a.events, a.pods
    ctx = pas_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream)
    req, mask, ncont, pods, nodes, cpc, cards = make_events(N, E, P, seed=0xC3)
    n_cards = np.full(N, K, np.int32)
    cap = np.tile(np.array([[8, 1000, 16_000_000_000, 100]], np.int64), (N, 1))
    zero = np.zeros((N, K, Q), np.int64)
    g_dev = (dev(n_cards), dev(cap), dev(zero))
    ev_dev = (dev(np.full(E, _lib.PAS_GAS_EV_ADD, np.int32)), dev(pods), dev(nodes))
    pod_dev = (dev(req), dev(mask), dev(ncont))
    ann_dev = (dev(cpc), dev(cards))
    st_t = torch.empty(E, dtype=torch.int32, device="cuda")
    gen = [10]

    def rebuild():
        gen[0] += 2
        ctx.gas_snapshot_set_device(gen[0], N, K, Q, *g_dev, stream)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        ctx.gas_apply_device(gen[0], gen[0] + 1, E, *ev_dev, P, C, *pod_dev, *ann_dev, LD, st_t,
                             stream=stream)
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    runs = [rebuild() for _ in range(a.warmup + a.steps)][a.warmup:]
    note(f"device rebuild: {stats(runs)}")
    assert int((st_t != _lib.PAS_GAS_OK).sum()) == 0
    _, dev_used = ctx.gas_snapshot_get()
    out = {"shape": {"nodes": N, "cards": K, "kinds": Q, "events": E, "containers": C,
                     "cards_ld": LD, "steps": a.steps, "warmup": a.warmup},
           "listed_cards": int(np.where(ncont[pods][:, None] > np.arange(C), cpc, 0).sum()),
           "apply_device": stats(runs)}
    if not a.no_host:
        host_ms, set_ms = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            used = host_rebuild(N, req, mask, ncont, pods, nodes, cpc, cards)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(used, dev_used), "device rebuild != host rebuild"
        for _ in range(a.warmup + a.steps):
            gen[0] += 2
            t0 = time.perf_counter()
            ctx.gas_snapshot_set(gen[0], n_cards, cap, used)
            set_ms.append((time.perf_counter() - t0) * 1e3)
        out["host_compute"] = stats(host_ms)
        out["snapshot_set_upload"] = stats(set_ms[a.warmup:])
        out["results_equal"] = True
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
