#!/usr/bin/env python3
"""Diagnostic: the deschedule step as a patch list against the dense masks (C4 shape).

Times pas_tas_deschedule_patches_device and pas_tas_deschedule_device on the same resident
inputs in one process: warm-up, then --steps timed steps of each, alternating, every step
between its own pair of HIP events on the launch stream; the medians are printed.  Two label
states:
  cold    no value bitmaps; carried labels chosen so that about 30 % of the nodes are listed
          (the nodes with a violation, topped up with nodes that carry a non-violated label);
  steady  the labels the cold patch leaves behind ("violating" where violated, "null" where a
          carried label was removed) with their value bitmaps, but for about 0.1 % of the
          nodes, whose values are unknown.
Also printed: the list lengths and the bytes a host reads per cycle (20 B per record + the two
counters, against 16 B per node of dense masks).  One JSON line per shape.

usage: patch_list_timing.py [--nodes 1000000] [--metrics 64] [--steps 30] [--warmup 5]
                            [--shapes 64x1,16x4]   (strategies x rules per strategy)
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
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype.fields:
        a = a.view(np.uint8)
    return torch.from_numpy(a).to("cuda")


def node_bits(nodes, n):
    """One bitmap row with the bits of `nodes` (bool [n]) set."""
    return wl.pack_bits(nodes[None, :])[0]


def median_ms(fns, steps, warmup, stream):
    """Median GPU ms of each callable, the callables alternating step by step."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(steps):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            f()
            e1.record(stream)
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in times]


def run_shape(ctx, snap, n, s, per, steps, warmup, stream):
    rules, off = wl.make_deschedule_rules(snap, s, per, seed=0xC4)
    viol = ctx.tas_violations(1, rules, off)
    violated = wl.unpack_bits(viol, n)            # [s][n]
    any_v = violated.any(axis=0)
    rng = np.random.default_rng(0xC4)
    # cold: top the listed nodes up to 30 % with carriers of strategy 0's (non-violated) label
    f_v = float(any_v.mean())
    p = max(0.0, (0.30 - f_v) / max(1.0 - f_v, 1e-9))
    carriers = ~any_v & (rng.random(n) < p)
    labels = np.zeros_like(viol)
    labels[0] = node_bits(carriers, n)
    # steady: what the cold patch leaves, values known but for 0.1 % of the nodes
    unknown = node_bits(rng.random(n) < 0.001, n)
    labels_after = labels | viol
    violating = viol & ~unknown[None, :]
    null = labels & ~viol & ~unknown[None, :]

    w = pas_amd.w64(n)
    rules_t, off_t = dev(rules), dev(off)
    viol_t = torch.empty((s, w), dtype=torch.int64, device="cuda")
    add_t = torch.empty(n, dtype=torch.int64, device="cuda")
    rem_t = torch.empty(n, dtype=torch.int64, device="cuda")
    total_t = torch.empty(1, dtype=torch.int64, device="cuda")
    node_t = torch.empty(n, dtype=torch.int32, device="cuda")
    padd_t = torch.empty(n, dtype=torch.int64, device="cuda")
    prem_t = torch.empty(n, dtype=torch.int64, device="cuda")
    n_t = torch.empty(1, dtype=torch.int64, device="cuda")
    ptotal_t = torch.empty(1, dtype=torch.int64, device="cuda")
    out = {"nodes": n, "strategies": s, "rules": len(rules), "steps": steps,
           "dense_bytes": 16 * n}
    for state, lab, vio, nul in (("cold", labels, None, None),
                                 ("steady", labels_after, violating, null)):
        lab_t = dev(lab)
        vio_t = None if vio is None else dev(vio)
        nul_t = None if nul is None else dev(nul)

        def dense():
            ctx.tas_deschedule_device(1, s, len(rules), rules_t, off_t, viol_t, lab_t, add_t,
                                      rem_t, total_t, stream)

        def patches():
            ctx.tas_deschedule_patches_device(1, s, len(rules), rules_t, off_t, lab_t, vio_t,
                                              nul_t, viol_t, n, node_t, padd_t, prem_t, n_t,
                                              ptotal_t, stream)

        def patches_ws():  # the sweep's bitmaps kept in the stream's workspace
            ctx.tas_deschedule_patches_device(1, s, len(rules), rules_t, off_t, lab_t, vio_t,
                                              nul_t, None, n, node_t, padd_t, prem_t, n_t,
                                              ptotal_t, stream)

        d_ms, p_ms, pw_ms = median_ms([dense, patches, patches_ws], steps, warmup, stream)
        n_p = int(n_t.item())
        assert int(ptotal_t.item()) == int(total_t.item())
        if vio is None:  # the list is the dense masks' non-zero nodes
            dense_nodes = torch.nonzero(add_t | rem_t).flatten().to(torch.int32)
            assert n_p == dense_nodes.numel() and torch.equal(node_t[:n_p], dense_nodes)
        out[state] = {"dense_ms": d_ms, "patches_ms": p_ms, "patches_workspace_viol_ms": pw_ms,
                      "n_patches": n_p, "listed_fraction": n_p / n,
                      "record_bytes": 20 * n_p + 16}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--metrics", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="64x1,16x4")
    a = ap.parse_args()
    ctx = pas_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream)
    snap = wl.make_tas_snapshot(a.nodes, a.metrics, seed=0xC4)
    ctx.tas_snapshot_set(1, snap.v_milli, snap.present)
    for shape in a.shapes.split(","):
        s, per = (int(x) for x in shape.split("x"))
        print(json.dumps(run_shape(ctx, snap, a.nodes, s, per, a.steps, a.warmup, stream)),
              flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
