#!/usr/bin/env python3
"""Diagnostic: what the wide merge records cost (DESIGN.md "Wide columns", recorded, not gated).

C5 shape on one GPU (65 536 pods x 1M nodes, k = 16), device events around each call, median
of --steps calls after --warmup (min - max beside it), all in one session:

  * pas_tas_gas_topk_device                          (the 64-bit records)
  * pas_tas_gas_topk_wide_device on the same narrow snapshot
  * pas_tas_gas_topk_wide_device with every fourth metric column wide, holding the same
    values (a quarter of the rules and of the pods' prioritize metrics land on them)
  * pas_topk_merge_device / pas_topk_merge_wide_device at 8 shards
  * pas_list_merge_device / pas_list_merge_wide_device at 8 x 12 544

The three C5 runs must give the same nodes and lengths (checked).  One JSON line.

usage: topk_wide_cost.py [--pods 65536] [--nodes 1000000] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "platform-aware-scheduling_amd"))

import pas_amd  # noqa: E402
from pas_amd import workload as wl  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def timed(fn, steps, warmup):
    """Median, min, max of the call's device time in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return {"median_us": float(np.median(us)), "min_us": min(us), "max_us": max(us)}


def sorted_runs(rng, S, P, w, wide):
    """[S][P][w] sorted runs of random records (keys from a small pool: the sub decides
    often), node ids distinct per pod."""
    keys = rng.integers(-50, 50, (S, P, w)).astype(np.int64)
    subs = rng.integers(0, 4, (S, P, w)).astype(np.int32) if wide else np.zeros((S, P, w),
                                                                               np.int32)
    nodes = np.empty((S, P, w), np.int32)
    for s in range(S):
        nodes[s] = np.arange(s * w, (s + 1) * w, dtype=np.int32)
    order = np.lexsort((nodes, subs.view(np.uint32), keys), axis=2)
    take = lambda a: np.take_along_axis(a, order, 2)  # noqa: E731
    return dev(take(keys)), dev(take(subs)), dev(take(nodes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=65_536)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--metrics", type=int, default=64)
    ap.add_argument("--rules", type=int, default=16)
    ap.add_argument("--topk", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    ctx.gas_snapshot_set(2, gs.n_cards, gs.cap, gs.used)
    t = (dev(batch.rules.view(np.uint8)), dev(batch.rule_off), dev(batch.prio.view(np.uint8)))
    g = (gb.req.shape[1], wl.I915, dev(gb.req), dev(gb.req_mask.view(np.int32)),
         dev(gb.n_containers))
    key = torch.empty((P, K), dtype=torch.int64, device="cuda")
    sub = torch.empty((P, K), dtype=torch.int32, device="cuda")
    node = torch.empty((P, K), dtype=torch.int32, device="cuda")
    ln = torch.empty(P, dtype=torch.int32, device="cuda")
    nr = len(batch.rules)

    def narrow(gen):
        return lambda: ctx.tas_gas_topk_device(gen, 2, P, nr, *t, None, *g, K, 0, key, node, ln,
                                               stream)

    def wide(gen):
        return lambda: ctx.tas_gas_topk_wide_device(gen, 2, P, nr, *t, None, *g, K, 0, key, sub,
                                                    node, ln, stream)

    out = {"shape": {"pods": P, "nodes": N, "metrics": M, "rules_per_pod": a.rules, "k": K,
                     "steps": a.steps, "warmup": a.warmup}}
    lists = []
    for name, fn in (("c5_narrow_entry", narrow(1)), ("c5_wide_entry_narrow_snapshot", wide(1))):
        out[name] = timed(fn, a.steps, a.warmup)
        lists.append((node.cpu().numpy().copy(), ln.cpu().numpy().copy()))
    cols = list(range(0, M, 4))
    v = snap.v_milli[cols]
    whole = np.floor_divide(v, 1000)
    nano = ((v - whole * 1000) * 10**6).astype(np.uint32)
    ctx.tas_snapshot_update_wide(1, 3, cols, whole, nano, snap.present[cols])
    out["wide_columns"] = len(cols)
    out["rules_on_wide_columns"] = float(np.isin(batch.rules["metric"], cols).mean())
    out["prio_on_wide_columns"] = float(np.isin(batch.prio["metric"], cols).mean())
    out["c5_wide_entry_quarter_wide"] = timed(wide(3), a.steps, a.warmup)
    lists.append((node.cpu().numpy().copy(), ln.cpu().numpy().copy()))
    for nd, le in lists[1:]:
        assert np.array_equal(le, lists[0][1]) and np.array_equal(nd, lists[0][0])
    out["lists_equal"] = True
    out["mean_list_len"] = float(lists[0][1].mean())

    rng = np.random.default_rng(0xC5)
    S = 8
    out_node = torch.empty((P, K), dtype=torch.int32, device="cuda")
    for name, w in (("topk_merge_8_shards", False), ("topk_merge_wide_8_shards", True)):
        ks, ss, ns = sorted_runs(rng, S, P, K, w)
        fn = (lambda: ctx.topk_merge_wide_device(P, K, S, ks, ss, ns, out_node, ln, stream)) if w \
            else (lambda: ctx.topk_merge_device(P, K, S, ks, ns, out_node, ln, stream))
        out[name] = timed(fn, a.steps, a.warmup)
    Pl, W = 512, 12_544
    out["list_merge_pods"] = Pl
    full = torch.empty((Pl, S * W), dtype=torch.int32, device="cuda")
    for name, w in (("list_merge_8x12544", False), ("list_merge_wide_8x12544", True)):
        ks, ss, ns = sorted_runs(rng, S, Pl, W, w)
        fn = (lambda: ctx.list_merge_wide_device(Pl, S, W, ks, ss, ns, full, ln[:Pl],
                                                 stream=stream)) if w \
            else (lambda: ctx.list_merge_device(Pl, S, W, ks, ns, full, ln[:Pl], stream=stream))
        out[name] = timed(fn, a.steps, a.warmup)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
