#!/usr/bin/env python3
"""Diagnostic: what the verbs by policy id cost against the routes they replace (DESIGN.md
"The resident policy table"; recorded, not gated on a ratio).

The C2 shape: 4096 pods x 100 000 nodes, 16 policies of 15 dontschedule rules and one
scheduleonmetric rule each, the pods spread evenly over the policies.

  eval     (a) pas_tas_eval_device with the pods' rules as per-pod CSRs (the parent's route)
           (b) pas_tas_eval_policies_device, warm: the violation bitmaps are cached
           (c) the same, cold: the first call after a column refresh, the sweep included (the
               refresh itself is outside the timed span)
           for PAS_TAS_FILTER alone and for FILTER | PRIORITIZE
  request  R = 256 requests of 1 000 nodes: pas_tas_filter_requests_device with per-request
           rule CSRs against pas_tas_filter_requests_policies_device (warm and cold)

Everything is resident on the device; a sample is the wall time of one call up to the end of
its stream.  The arms alternate, --repeats times: median, min - max.  The outputs of the routes
are compared equal at the timed sizes first.  One JSON line.

usage: policy_eval_cost.py [--nodes 100000] [--pods 4096] [--repeats 7] [--warmup 2]
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
from pas_amd import workload as wl  # noqa: E402
from pas_amd.context import w64  # noqa: E402


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4),
            "max_ms": round(float(max(ms)), 4)}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(arms, repeats, warmup, before=None):
    """Per-call milliseconds of the arms, alternated; before[name] runs untimed ahead of
    every call of that arm."""
    before = before or {}
    out = {name: [] for name in arms}
    for k in range(warmup + repeats):
        for name, fn in arms.items():
            if name in before:
                before[name]()
            ms = timed(fn)
            if k >= warmup:
                out[name].append(ms)
    return {name: stats(ms) for name, ms in out.items()}


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype.names:  # pas_rule records as bytes
        a = a.view(np.uint8)
    return torch.from_numpy(a).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--metrics", type=int, default=8)
    ap.add_argument("--pods", type=int, default=4096)
    ap.add_argument("--policies", type=int, default=16)
    ap.add_argument("--rules", type=int, default=15)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--req", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    N, P, K, W = a.nodes, a.pods, a.policies, w64(a.nodes)
    s = torch.cuda.current_stream()
    ctx = pas_amd.Context(0)
    snap = wl.make_tas_snapshot(N, a.metrics, seed=0xE1)
    ctx.tas_snapshot_set(1, snap.v_milli, snap.present)
    gen = [1]
    table = wl.make_tas_batch(snap, K, a.rules, seed=0xE2)  # K policies as K "pods"
    ctx.tas_policies_set(table.rules, table.rule_off, table.prio)
    col_v, col_p = dev(snap.v_milli[:1]), dev(snap.present[:1])

    def refresh():  # a column refresh with the same values: the generation moves
        ctx.tas_snapshot_update_device(gen[0], gen[0] + 1, [0], col_v, col_p, stream=s)
        gen[0] += 1

    def per_item(ids):  # the per-pod / per-request CSR of the parent's routes
        rows = [table.rules[table.rule_off[i]: table.rule_off[i + 1]] for i in ids]
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        return np.concatenate(rows), off

    result = {"nodes": N, "pods": P, "policies": K, "rules_per_policy": a.rules,
              "repeats": a.repeats, "eval": {}, "request_filter": {}}

    ids = (np.arange(P) % K).astype(np.int32)
    rules, off = per_item(ids)
    rules_t, off_t, prio_t, ids_t = dev(rules), dev(off), dev(table.prio[ids]), dev(ids)
    pass_a = torch.zeros((P, W), dtype=torch.int64, device="cuda")
    pass_b = torch.zeros((P, W), dtype=torch.int64, device="cuda")
    order_a = torch.zeros((P, N), dtype=torch.int32, device="cuda")
    order_b = torch.zeros((P, N), dtype=torch.int32, device="cuda")
    len_a = torch.zeros(P, dtype=torch.int32, device="cuda")
    len_b = torch.zeros(P, dtype=torch.int32, device="cuda")
    for flags, name in ((1, "filter"), (3, "filter_prioritize")):
        def per_pod():
            ctx.tas_eval_device(gen[0], P, len(rules), rules_t, off_t, prio_t, None, flags,
                                pass_a, order_a, len_a, stream=s)

        def by_policy():
            ctx.tas_eval_policies_device(gen[0], P, ids_t, None, flags, pass_b, order_b, len_b,
                                         stream=s)

        per_pod()
        by_policy()
        torch.cuda.synchronize()
        assert torch.equal(pass_a, pass_b), "pass rows differ between the routes"
        if flags & 2:
            assert torch.equal(len_a, len_b), "list lengths differ between the routes"
            keep = torch.arange(N, device="cuda")[None, :] < len_a[:, None]
            assert torch.equal(order_a * keep, order_b * keep), "lists differ between the routes"
            del keep
        result["eval"][name] = alternate(
            {"per_pod_rules": per_pod, "by_policy_warm": by_policy, "by_policy_cold": by_policy},
            a.repeats, a.warmup, before={"by_policy_cold": refresh})

    rng = np.random.default_rng(0xE3)
    R, n = a.requests, a.req
    req = np.concatenate([rng.permutation(N)[:n] for _ in range(R)]).astype(np.int32)
    req_off = (np.arange(R + 1) * n).astype(np.int32)
    rids = (np.arange(R) % K).astype(np.int32)
    rrules, rrule_off = per_item(rids)
    req_t, rrules_t, rrule_off_t = dev(req), dev(rrules), dev(rrule_off)
    ld = w64(n)
    rows_a = torch.zeros((R, ld), dtype=torch.int64, device="cuda")
    rows_b = torch.zeros((R, ld), dtype=torch.int64, device="cuda")

    def req_rules():
        ctx.tas_filter_requests_device(gen[0], req_off, len(rrules), rrules_t, rrule_off_t,
                                       req_t, rows_a, ld, stream=s)

    def req_policy():
        ctx.tas_filter_requests_policies_device(gen[0], req_off, rids, req_t, rows_b, ld,
                                                stream=s)

    req_rules()
    req_policy()
    torch.cuda.synchronize()
    assert torch.equal(rows_a, rows_b), "request rows differ between the routes"
    result["request_filter"] = {"requests": R, "req_nodes": n}
    result["request_filter"].update(alternate(
        {"per_request_rules": req_rules, "by_policy_warm": req_policy,
         "by_policy_cold": req_policy}, a.repeats, a.warmup, before={"by_policy_cold": refresh}))
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
