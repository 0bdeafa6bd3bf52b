"""Batch placement to completion: top-k rows and placement, round after round, until every
pod is placed or has tried every node of its list.

One pas_tas_gas_topk_device -> pas_gas_place_device pass leaves a pod unplaced as soon as its
k candidates were taken by the pods before it.  Here such a pod continues: its next row
resumes the list strictly after the last record it tried (pas_tas_gas_topk[_wide]_after_device
or, by policy id, pas_tas_gas_topk_policies[_wide]_after_device; include/pas.h "Resuming a
top-k list") on the usage the round before left behind.

Equivalence.  During the call the usage only grows, so a node that did not fit a pod at a
round's start never fits it later in the call: a row holds the next k nodes of the pod's list
that can still take it.  Each round is therefore the sequential pod-after-pod loop of
pas_gas_place over the queued pods, each walking its full list from its cursor for at most k
still-feasible nodes, and a pod that used up its k goes to the back of the queue, as a pod that
failed to bind does in kube-scheduler (the extender is called again and answers from its
current cache).  A pod ends unplaced only when a row came back shorter than k, i.e. when every
node of its list had been tried or no longer fits.  The caller must not interleave releases or
node / pod events with the call: they would let a node the cursor has passed fit again.

Torch allocates the buffers and does the elementwise plumbing between the two device calls;
there is no per-pod work on the host."""
from collections import namedtuple

import torch

from ._lib import PAS_ECAPACITY, PasError

INT32_MAX = 2**31 - 1
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1

PlacementResult = namedtuple("PlacementResult", "node round res n_placed rounds gas_gen")
PlacementResult.__doc__ = """place_to_completion's result: node int32 [P] (global id, -1 =
unplaced), round int32 [P] (0-based round the pod was placed in, -1 = unplaced), res int32 [P]
(pas_gas_place_device's result word, 0 for an unplaced pod), all on the device; n_placed,
rounds (top-k + place passes run) and gas_gen (the GAS generation after the last pass)."""

AnnotatedPlacement = namedtuple("AnnotatedPlacement",
                                PlacementResult._fields + ("status", "ann_off", "ann_bytes",
                                                           "node_off", "node_bytes"))
AnnotatedPlacement.__doc__ = """place_to_completion(annotate=True)'s result: PlacementResult's
fields, then what bindNode writes per pod, rendered on the device
(pas_gas_annotations_render_device, pas_names_render_device): status int32 [P] (PAS_GAS_OK for every pod of a sound placement),
pod p's "gas-container-cards" value ann_bytes[ann_off[p]:ann_off[p + 1]] and its node's name
node_bytes[node_off[p]:node_off[p + 1]] (the Binding's target), both empty for an unplaced pod;
offsets int64 [P + 1], bytes uint8, all on the device."""


def place_to_completion(ctx, tas_gen: int, gas_gen: int, n_pods: int, n_rules: int, rules_t,
                        rule_off_t, prio_t, cand_t, max_containers: int, i915_index: int, req_t,
                        mask_t, ncont_t, k: int, node_base: int = 0, wide: bool = False,
                        max_rounds=None, stream=None, pod_policy_t=None, annotate: bool = False):
    """Place a batch until every pod is placed or has provably run out of nodes (the module's
    docstring has the equivalence).  The pod batch tensors are those of
    Context.tas_gas_topk[_wide]_device and Context.gas_place_device; wide selects the wide
    records (required on a snapshot with wide columns).  Every pass moves the GAS snapshot one
    generation on, from gas_gen; the result names the last one.

    pod_policy_t (int32 [P] on the device): the pods name rows of the resident policy table
    and every round calls pas_tas_gas_topk_policies[_wide]_after_device; n_rules, rules_t,
    rule_off_t and prio_t are then ignored and may be None.  The policies' violating sets are
    built at most once per call, by the first round if they are not current: the TAS snapshot
    does not change between rounds, so the later rounds evaluate no dontschedule rule at all.

    max_rounds defaults to ceil(N / k) + 1, which the loop cannot exceed: every unfinished
    cursor advances by k records per round.  Passing it raises RuntimeError (the passes run so
    far stay committed, the snapshot is at gas_gen + max_rounds).  Errors of the two device
    calls propagate as PasError: a stale generation before anything changed, PAS_EDEVICE from
    the place call as pas_gas_place_device reports it.

    annotate: every round also takes the selections as counts per container and card, and after
    the last round one pas_gas_annotations_render_device and one pas_names_render_device call
    turn the batch into the strings the shim writes (the card-name table and the name table must
    be resident); the result is an AnnotatedPlacement.  Without it nothing changes: the same
    device calls, a PlacementResult."""
    stream = torch.cuda.current_stream() if stream is None else stream
    if max_rounds is None:
        max_rounds = -(-ctx.gas_shape[0] // k) + 1
    with torch.cuda.stream(stream):
        dev = req_t.device if req_t is not None else "cuda"

        def full(shape, value, dtype):
            return torch.full(shape, value, dtype=dtype, device=dev)
        p = n_pods
        # the cursors: begin for every pod
        after_key, after_node = full((p,), INT64_MIN, torch.int64), full((p,), -1, torch.int32)
        after_sub = full((p,), 0, torch.int32) if wide else None
        node, rnd = full((p,), -1, torch.int32), full((p,), -1, torch.int32)
        res = full((p,), 0, torch.int32)
        key = torch.empty((p, k), dtype=torch.int64, device=dev)
        sub = torch.empty((p, k), dtype=torch.int32, device=dev) if wide else None
        top_node = torch.empty((p, k), dtype=torch.int32, device=dev)
        top_len = torch.empty(p, dtype=torch.int32, device=dev)
        r_node = torch.empty(p, dtype=torch.int32, device=dev)
        r_rank = torch.empty(p, dtype=torch.int32, device=dev)
        r_res = torch.empty(p, dtype=torch.int32, device=dev)
        if annotate:
            shape = (p, max_containers, ctx.gas_shape[1])
            r_counts = torch.empty(shape, dtype=torch.int64, device=dev)
            counts = torch.zeros(shape, dtype=torch.int64, device=dev)
        else:
            r_counts = None
        gen, rounds, n_placed = gas_gen, 0, 0
        while True:
            if rounds >= max_rounds:
                raise RuntimeError(f"place_to_completion: pods still queued after {rounds} "
                                   f"rounds (max_rounds)")
            tail = (cand_t, max_containers, i915_index, req_t, mask_t, ncont_t, k, node_base)
            if pod_policy_t is not None:
                head = (tas_gen, gen, p, pod_policy_t) + tail
                topk = ctx.tas_gas_topk_policies_after_device
                topk_wide = ctx.tas_gas_topk_policies_wide_after_device
            else:
                head = (tas_gen, gen, p, n_rules, rules_t, rule_off_t, prio_t) + tail
                topk = ctx.tas_gas_topk_after_device
                topk_wide = ctx.tas_gas_topk_wide_after_device
            if wide:
                topk_wide(*head, after_key, after_sub, after_node, key, sub, top_node, top_len,
                          stream=stream)
            else:
                topk(*head, after_key, after_node, key, top_node, top_len, stream=stream)
            placed_now, _ = ctx.gas_place_device(gen, gen + 1, p, max_containers, i915_index,
                                                 req_t, mask_t, ncont_t, k, k, node_base,
                                                 top_node, top_len, r_node, r_rank, r_res,
                                                 counts_t=r_counts, stream=stream)
            gen += 1
            n_placed += placed_now
            if p == 0:
                rounds += 1
                break
            placed = r_node >= 0
            node = torch.where(placed, r_node, node)
            res = torch.where(placed, r_res, res)
            rnd = torch.where(placed, torch.full_like(rnd, rounds), rnd)
            if annotate:
                counts = torch.where(placed[:, None, None], r_counts, counts)
            rounds += 1
            # the next cursors: the end for a placed pod, the row's last record otherwise (the
            # padding record, i.e. the end, when the row was shorter than k)
            after_key = torch.where(placed, torch.full_like(after_key, INT64_MAX), key[:, k - 1])
            after_node = torch.where(placed, torch.full_like(after_node, INT32_MAX),
                                     top_node[:, k - 1])
            if wide:
                after_sub = torch.where(placed, torch.full_like(after_sub, -1), sub[:, k - 1])
            # queued: unplaced with a full row (finished pods come back with an empty row)
            if not bool((~placed & (top_len == k)).any()):
                break
        result = PlacementResult(node, rnd, res, n_placed, rounds, gen)
        if not annotate:
            return result
        # the strings: one render of the annotations and one of the names
        bind_node = torch.where(node >= 0, node - node_base, torch.full_like(node, -1))
        status = torch.zeros(max(p, 1), dtype=torch.int32, device=dev)[:p]
        ann_off = torch.zeros(p + 1, dtype=torch.int64, device=dev)
        node_off = torch.zeros(p + 1, dtype=torch.int64, device=dev)

        def rendered(call, room):
            # one call when the guessed room holds the bytes, else a second with the exact room
            out = torch.empty(max(room, 1), dtype=torch.uint8, device=dev)
            try:
                total = call(out, room)
            except PasError as e:
                if e.code != PAS_ECAPACITY:
                    raise
                total = e.n_bytes
                out = torch.empty(total, dtype=torch.uint8, device=dev)
                call(out, total)
            return out[:total]
        ann_bytes = rendered(lambda out, cap: ctx.gas_annotations_render_device(
            p, bind_node, ncont_t, max_containers, counts, status, ann_off, out, cap,
            stream=stream), 32 * p * max(max_containers, 1))
        node_bytes = rendered(lambda out, cap: ctx.names_render_device(
            p, node, node_base, node_off, out, cap, stream=stream), 64 * p)
        return AnnotatedPlacement(*result, status, ann_off, ann_bytes, node_off, node_bytes)
