#!/usr/bin/env python3
"""Diagnostic: what resuming a top-k list costs and what placing to completion buys
(DESIGN.md §3 "Resumed lists and placement to completion"; recorded, not gated on a time).

C5 shape on one GPU (65 536 pods x 1M nodes, k = 16), the bench's C5 inputs.  Medians of --steps
after --warmup, min - max beside them:

  topk           pas_tas_gas_topk_device                                  (device time, events)
  after_begin    pas_tas_gas_topk_after_device with the begin cursor: the same records (checked);
                 the difference to topk is the start search plus one launch
  after_page2    the same call with each pod's last record of the first page as its cursor
  topk_place     today's single pass: topk, then pas_gas_place_device      (wall time)
  complete       placement.place_to_completion: rounds, pods placed per round, wall time; the
                 GAS snapshot is uploaded again outside the timed region before each run

One JSON line.

usage: place_complete_cost.py [--pods 65536] [--nodes 1000000] [--steps 20] [--warmup 3]
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
from pas_amd.placement import place_to_completion  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=65_536)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--metrics", type=int, default=64)
    ap.add_argument("--rules", type=int, default=16)
    ap.add_argument("--topk", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-rounds", type=int, default=400)
    a = ap.parse_args()
    P, N, M, K = a.pods, a.nodes, a.metrics, a.topk
    ctx = pas_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream)
    snap = wl.make_tas_snapshot(N, M, seed=0xC5)
    batch = wl.make_tas_batch(snap, P, a.rules - 1, seed=0xC5)
    gs = wl.make_gas_snapshot(N, seed=0xC5)
    gb = wl.make_gas_batch(P, seed=0xC5)
    ctx.tas_snapshot_set(1, snap.v_milli, snap.present)
    kc, q = gs.used.shape[1:]
    g_dev = (dev(gs.n_cards), dev(gs.cap), dev(gs.used))
    gen = [10]

    def upload():
        gen[0] += a.max_rounds + 2
        ctx.gas_snapshot_set_device(gen[0], N, kc, q, *g_dev, stream)
        torch.cuda.synchronize()
        return gen[0]

    C = gb.req.shape[1]
    tas = (len(batch.rules), dev(batch.rules.view(np.uint8)), dev(batch.rule_off),
           dev(batch.prio.view(np.uint8)), None)
    gas = (C, wl.I915, dev(gb.req), dev(gb.req_mask.view(np.int32)), dev(gb.n_containers))
    key = torch.empty((P, K), dtype=torch.int64, device="cuda")
    top_node = torch.empty((P, K), dtype=torch.int32, device="cuda")
    top_len = torch.empty(P, dtype=torch.int32, device="cuda")
    note("inputs ready")
    g0 = upload()

    def timed(fn):
        """Device time of fn's launches on the stream, per run."""
        ms = []
        for _ in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return stats(ms[a.warmup:])

    def topk():
        ctx.tas_gas_topk_device(1, g0, P, *tas, *gas, K, 0, key, top_node, top_len, stream)

    def after(ck, cn):
        return lambda: ctx.tas_gas_topk_after_device(1, g0, P, *tas, *gas, K, 0, ck, cn, key,
                                                      top_node, top_len, stream)

    out = {"shape": {"pods": P, "nodes": N, "k": K, "steps": a.steps, "warmup": a.warmup}}
    out["topk"] = timed(topk)
    first = (key.clone(), top_node.clone(), top_len.clone())
    begin = (torch.full((P,), -2**63, dtype=torch.int64, device="cuda"),
             torch.full((P,), -1, dtype=torch.int32, device="cuda"))
    out["after_begin"] = timed(after(*begin))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, (key, top_node, top_len)))
    out["after_begin_equals_topk"] = True
    page2 = (first[0][:, K - 1].contiguous(), first[1][:, K - 1].contiguous())
    out["after_page2"] = timed(after(*page2))
    torch.cuda.synchronize()
    out["after_page2"]["mean_row_len"] = float(top_len.float().mean())
    out["topk"]["mean_row_len"] = float(first[2].float().mean())
    note(f"top-k: {out['topk']} {out['after_begin']} {out['after_page2']}")

    node_t = torch.empty(P, dtype=torch.int32, device="cuda")
    rank_t = torch.empty(P, dtype=torch.int32, device="cuda")
    res_t = torch.empty(P, dtype=torch.int32, device="cuda")

    def topk_place():
        g = upload()
        t0 = time.perf_counter()
        ctx.tas_gas_topk_device(1, g, P, *tas, *gas, K, 0, key, top_node, top_len, stream)
        placed, _ = ctx.gas_place_device(g, g + 1, P, *gas, K, K, 0, top_node, top_len, node_t,
                                         rank_t, res_t, stream=stream)
        return (time.perf_counter() - t0) * 1e3, placed

    runs = [topk_place() for _ in range(a.warmup + a.steps)][a.warmup:]
    out["topk_place"] = dict(stats([r[0] for r in runs]), placed=runs[-1][1])
    note(f"topk_place: {out['topk_place']}")

    def complete():
        g = upload()
        t0 = time.perf_counter()
        r = place_to_completion(ctx, 1, g, P, *tas, *gas, K, max_rounds=a.max_rounds,
                                stream=stream)
        return (time.perf_counter() - t0) * 1e3, r

    runs = [complete() for _ in range(a.warmup + a.steps)][a.warmup:]
    r = runs[-1][1]
    rnd = r.round.cpu().numpy()
    out["complete"] = dict(stats([x[0] for x in runs]), placed=r.n_placed, rounds=r.rounds,
                           placed_per_round=np.bincount(rnd[rnd >= 0],
                                                        minlength=r.rounds).tolist())
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
