#!/usr/bin/env python3
"""Diagnostic: the C5 top-k by policy id against the per-pod rules form (DESIGN.md §3 "Top-k by
policy id"; recorded, not gated on a ratio).

The C5 shape of bench.py: 65 536 pods x 1M nodes x 64 metrics, 15 dontschedule rules and one
scheduleonmetric rule per pod, 8 cards x 3 kinds, k = 16, pas_amd.workload's generators with
bench.py's seed.  The pods' rule sets become the policy table:

  --policies 0   the distinct (rules, prio) sets of the pods themselves.  The generator draws
                 every pod's rules independently, so this is one policy per pod: the worst case
                 for the table (viol holds n_policies x N bits).
  --policies D   D policies drawn by the same generator, pod p on policy p % D: a cluster
                 whose pods share a few dozen TASPolicy objects.  Both arms run these rules.

Arms, alternated --steps times after --warmup (median, min - max):
  rules     pas_tas_gas_topk_device with the per-pod CSR and prio
  policies  pas_tas_gas_topk_policies_device, the violating sets already built
as the kernel time of PAS_K_TAS_GAS_TOPK (pas_set_timing(2) / pas_kernel_time) and as the wall
time of the call up to the end of its stream.  One-off costs, wall time of the first call after
a column refresh minus the arm's warm median, --cold times:
  rules     the node-major copies' transposes (vals_t, pres_t)
  policies  the violating sets' sweep (its kernel time beside it, PAS_K_TAS_VIOLATIONS)
The outputs of the two arms are compared equal first.  One JSON line.

usage: topk_policies_cost.py [--policies 0] [--steps 20] [--warmup 3] [--cold 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "platform-aware-scheduling_amd"))

import torch  # noqa: E402

import pas_amd  # noqa: E402
from pas_amd import _lib  # noqa: E402
from pas_amd import workload as wl  # noqa: E402
from pas_amd.context import w64  # noqa: E402


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4),
            "max_ms": round(float(max(ms)), 4)}


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype.names:  # pas_rule records as bytes
        a = a.view(np.uint8)
    return torch.from_numpy(a).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=65_536)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--metrics", type=int, default=64)
    ap.add_argument("--rules", type=int, default=16, help="per pod, the prio rule included")
    ap.add_argument("--topk", type=int, default=16)
    ap.add_argument("--policies", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cold", type=int, default=3)
    a = ap.parse_args()
    P, N, M, R, K = a.pods, a.nodes, a.metrics, a.rules - 1, a.topk
    s = torch.cuda.current_stream()
    ctx = pas_amd.Context(0)
    ctx.set_stream(s)
    snap = wl.make_tas_snapshot(N, M, seed=0xC5)
    ctx.tas_snapshot_set(1, snap.v_milli, snap.present)
    gen = [1]
    col_v, col_p = dev(snap.v_milli[:1]), dev(snap.present[:1])
    if a.policies > 0:
        table = wl.make_tas_batch(snap, a.policies, R, seed=0xC5)
        ids = (np.arange(P) % a.policies).astype(np.int32)
    else:  # the pods' own rule sets, made distinct
        pods = wl.make_tas_batch(snap, P, R, seed=0xC5)
        rows = np.concatenate([pods.rules.view(np.uint8).reshape(P, -1),
                               pods.prio.view(np.uint8).reshape(P, -1)], axis=1)
        _, first, ids = np.unique(rows, axis=0, return_index=True, return_inverse=True)
        ids = ids.reshape(-1).astype(np.int32)
        take = (first[:, None] * R + np.arange(R)[None, :]).reshape(-1)
        table = wl.TasBatch(pods.rules[take], (np.arange(len(first) + 1) * R).astype(np.int32),
                            pods.prio[first])
    D = len(table.prio)
    del snap
    ctx.tas_policies_set(table.rules, table.rule_off, table.prio)
    # the per-pod CSR of the same rules
    take = (ids.astype(np.int64)[:, None] * R + np.arange(R)[None, :]).reshape(-1)
    rules_t, prio_t = dev(table.rules[take]), dev(table.prio[ids])
    off_t = dev((np.arange(P + 1, dtype=np.int64) * R).astype(np.int32))
    ids_t = dev(ids)
    n_rules = P * R
    gsnap = wl.make_gas_snapshot(N, seed=0xC5)
    ctx.gas_snapshot_set(2, gsnap.n_cards, gsnap.cap, gsnap.used)
    cards, kinds = gsnap.used.shape[1], gsnap.used.shape[2]
    del gsnap
    gb = wl.make_gas_batch(P, seed=0xC5)
    gas = (gb.req.shape[1], wl.I915, dev(gb.req), dev(gb.req_mask), dev(gb.n_containers))

    def outputs():
        return (torch.zeros((P, K), dtype=torch.int64, device="cuda"),
                torch.zeros((P, K), dtype=torch.int32, device="cuda"),
                torch.zeros(P, dtype=torch.int32, device="cuda"))
    out_r, out_p = outputs(), outputs()

    def by_rules():
        ctx.tas_gas_topk_device(gen[0], 2, P, n_rules, rules_t, off_t, prio_t, None, *gas, K, 0,
                                *out_r, stream=s)

    def by_policy():
        ctx.tas_gas_topk_policies_device(gen[0], 2, P, ids_t, None, *gas, K, 0, *out_p, stream=s)

    def refresh():  # a column refresh with the same values: the derived data is stale
        ctx.tas_snapshot_update_device(gen[0], gen[0] + 1, [0], col_v, col_p, stream=s)
        gen[0] += 1

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def kernel(fn, kid):
        ctx.reset_timing()
        ms = wall(fn)
        k_ms, k_n = ctx.kernel_time(kid)
        return ms, k_ms, k_n

    ctx.set_timing(2)
    arms = {"rules": by_rules, "policies": by_policy}
    first = {name: wall(fn) for name, fn in arms.items()}  # (allocations included)
    for x, y, what in zip(out_r, out_p, ("key", "node", "len")):
        assert torch.equal(x, y), f"{what} differs between the two forms"
    entries = int(out_p[2].to(torch.int64).sum().item())
    warm = {name: {"kernel": [], "wall": []} for name in arms}
    for i in range(a.warmup + a.steps):
        for name, fn in arms.items():
            ms, k_ms, k_n = kernel(fn, _lib.PAS_K_TAS_GAS_TOPK)
            assert k_n == 1, k_n
            if i >= a.warmup:
                warm[name]["kernel"].append(k_ms)
                warm[name]["wall"].append(ms)
    cold = {name: [] for name in arms}
    sweep = []
    for _ in range(a.cold):
        for name, fn in arms.items():
            refresh()
            ms, _, _ = kernel(fn, _lib.PAS_K_TAS_GAS_TOPK)
            cold[name].append(ms - float(np.median(warm[name]["wall"])))
            if name == "policies":
                sweep.append(ctx.kernel_time(_lib.PAS_K_TAS_VIOLATIONS)[0])
    ctx.set_timing(0)
    result = {
        "pods": P, "nodes": N, "metrics": M, "rules_per_pod": R + 1, "topk": K, "cards": cards,
        "kinds": kinds, "distinct_policies": D, "steps": a.steps, "entries": entries,
        "first_call_wall_ms": {k: round(v, 3) for k, v in first.items()},
        "topk_kernel": {name: stats(warm[name]["kernel"]) for name in arms},
        "call_wall": {name: stats(warm[name]["wall"]) for name in arms},
        "one_off": {"rules_transposes_wall": stats(cold["rules"]),
                    "policies_viol_build_wall": stats(cold["policies"]),
                    "policies_viol_sweep_kernel": stats(sweep)},
        "device_bytes": {"vals_t_pres_t_not_held": 8 * N * M + 8 * N * ((M + 63) // 64),
                         "viol_held": 8 * D * w64(N)},
    }
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
