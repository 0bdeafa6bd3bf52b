#!/usr/bin/env python3
"""Diagnostic: what the batch placement costs (DESIGN.md §3 "Batch placement", recorded, not
gated on a time).

C5 shape on one GPU (65 536 pods x 1M nodes): the bench's C5 inputs go through
pas_tas_gas_topk_device (k = 16) once, and pas_gas_place_device places the rows.  The call is
synchronous, so its cost is wall time: median of --steps calls after --warmup (min - max
beside it), the GAS snapshot uploaded again outside the timed region before each call (the
call changes it).  Beside it: device rounds, pods placed, and the longest run and round count
of a host model of the rounds fed with the call's own result (the model's round count must
equal the call's).

Baseline, same session: the only other route to the same placements, the loop of pas.h as
single-pair pas_gas_bind calls, on the first --prefix pods; the new call is timed on the same
prefix and must give the same placements and usage (checked) in no more time (checked).
One JSON line.

usage: gas_place_cost.py [--pods 65536] [--nodes 1000000] [--prefix 1024] [--steps 20]
                         [--warmup 3]
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
from pas_amd import workload as wl  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def model_rounds(rows, lens, n_nodes, rank):
    """The node-centric rounds on the host, fed with each pod's final rank (-1: the pod tries
    its whole row): (rounds, longest run).  A run is the pods one node's owner processes in a
    round."""
    P, k = rows.shape
    col = np.arange(k)[None, :]
    valid = (col < np.clip(lens, 0, k)[:, None]) & (rows >= 0) & (rows < n_nodes)
    pod = np.arange(P)
    first = np.where(valid.any(1), valid.argmax(1), -1)
    cur = first.copy()
    rounds = longest = 0
    while (cur >= 0).any():
        rounds += 1
        act = cur >= 0
        blocker = np.full(n_nodes, P, np.int64)
        later = valid & (col > cur[:, None]) & act[:, None]
        np.minimum.at(blocker, rows[later], np.broadcast_to(pod[:, None], rows.shape)[later])
        node = rows[pod, np.maximum(cur, 0)]
        go = act & (pod <= blocker[np.where(act, node, 0)])
        longest = max(longest, int(np.bincount(node[go]).max()))
        nxt = np.where(valid & (col > cur[:, None]), col, k).min(1)
        nxt = np.where(nxt < k, nxt, -1)
        cur = np.where(go, np.where(cur == rank, -1, nxt), cur)
    return rounds, longest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=65_536)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--metrics", type=int, default=64)
    ap.add_argument("--rules", type=int, default=16)
    ap.add_argument("--topk", type=int, default=16)
    ap.add_argument("--prefix", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    P, N, M, K = a.pods, a.nodes, a.metrics, a.topk
    pre = min(a.prefix, P)
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
        gen[0] += 2
        ctx.gas_snapshot_set_device(gen[0], N, kc, q, *g_dev, stream)
        torch.cuda.synchronize()
        return gen[0]

    C = gb.req.shape[1]
    req_t, mask_t, nc_t = dev(gb.req), dev(gb.req_mask.view(np.int32)), dev(gb.n_containers)
    key = torch.empty((P, K), dtype=torch.int64, device="cuda")
    top_node = torch.empty((P, K), dtype=torch.int32, device="cuda")
    top_len = torch.empty(P, dtype=torch.int32, device="cuda")
    g0 = upload()
    ctx.tas_gas_topk_device(1, g0, P, len(batch.rules), dev(batch.rules.view(np.uint8)),
                            dev(batch.rule_off), dev(batch.prio.view(np.uint8)), None, C, wl.I915,
                            req_t, mask_t, nc_t, K, 0, key, top_node, top_len, stream)
    torch.cuda.synchronize()
    rows, lens = top_node.cpu().numpy(), top_len.cpu().numpy()
    note("rows ready")
    node_t = torch.empty(P, dtype=torch.int32, device="cuda")
    rank_t = torch.empty(P, dtype=torch.int32, device="cuda")
    res_t = torch.empty(P, dtype=torch.int32, device="cuda")

    def place(n_pods):
        """One timed placement of the first n_pods rows: (ms, placed, rounds)."""
        g = upload()
        t0 = time.perf_counter()
        placed, rounds = ctx.gas_place_device(g, g + 1, n_pods, C, wl.I915, req_t, mask_t, nc_t, K,
                                              K, 0, top_node, top_len, node_t, rank_t, res_t,
                                              stream=stream)
        return (time.perf_counter() - t0) * 1e3, placed, rounds

    def bind_loop(n_pods):
        """The same placements as single-pair pas_gas_bind calls: (ms, nodes, calls)."""
        g = upload()
        req, mask, nc = gb.req[:n_pods], gb.req_mask[:n_pods], gb.n_containers[:n_pods]
        nodes = np.full(n_pods, -1, np.int32)
        calls = 0
        t0 = time.perf_counter()
        for p in range(n_pods):
            for j in range(min(K, int(lens[p]))):
                n = int(rows[p, j])
                if n < 0 or n >= N:
                    continue
                _, st = ctx.gas_bind(g, g + 1, [p], [n], req, mask, nc, wl.I915)
                g += 1
                calls += 1
                if st[0] == _lib.PAS_GAS_OK:
                    nodes[p] = n
                    break
        gen[0] = g + 1
        return (time.perf_counter() - t0) * 1e3, nodes, calls

    out = {"shape": {"pods": P, "nodes": N, "k": K, "prefix": pre, "steps": a.steps,
                     "warmup": a.warmup}, "mean_row_len": float(lens.mean())}
    for name, n_pods in (("place_full", P), ("place_prefix", pre)):
        runs = [place(n_pods) for _ in range(a.warmup + a.steps)][a.warmup:]
        note(f"{name}: {runs[-1]}")
        rank = rank_t.cpu().numpy()[:n_pods]
        m_rounds, longest = model_rounds(rows[:n_pods], lens[:n_pods], N, rank)
        assert m_rounds == runs[-1][2], (m_rounds, runs[-1][2])
        out[name] = dict(stats([r[0] for r in runs]), placed=runs[-1][1], rounds=runs[-1][2],
                         longest_run=longest, placed_past_first=int((rank > 0).sum()))
    place_nodes = node_t.cpu().numpy()[:pre].copy()
    _, place_used = ctx.gas_snapshot_get()
    loops = [bind_loop(pre) for _ in range(a.warmup + a.steps)][a.warmup:]
    _, loop_used = ctx.gas_snapshot_get()
    note("bind loop done")
    assert np.array_equal(loops[-1][1], place_nodes) and np.array_equal(loop_used, place_used)
    out["bind_loop_prefix"] = dict(stats([r[0] for r in loops]), calls=loops[-1][2])
    out["prefix_results_equal"] = True
    out["place_not_slower_than_loop"] = (out["place_prefix"]["median_ms"]
                                         <= out["bind_loop_prefix"]["median_ms"])
    print(json.dumps(out))
    ctx.close()
    assert out["place_not_slower_than_loop"]


if __name__ == "__main__":
    main()
