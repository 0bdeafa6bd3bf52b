"""Pod events from annotation strings (pas_gas_annotations_resolve, pas_gas_apply_annotations
and their _names / _device forms, csrc/gas_annotations.hip).

The reference answer has two layers.  The route the cache took so far is restated on the host:
snapshot.parse_annotation per event, errBadArgs / the unknown node / the annotation without cards
settled there as GasCache._plan settles them, and pas_gas_apply (on a second context) for the
rest.  Under it lies test_gas_apply.ref_apply, the oracle's adjustPodResources loop, for the
events that reach the walker.  The generated batches assert on themselves that they reach every
outcome; that part needs no GPU.

Shapes: N = 65 node slots of which 40 are live, Q = 3, C = 3, k in {8, 16, 64} (the walker's
three card tiers; "card1" / "card10" are prefixes of each other from 11 cards on)."""
import functools

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd.snapshot import go_sort_strings, pack_names, parse_annotation
from test_gas_apply import (ADD, C, ERR_INPUT, ERR_OVERFLOW, I64_MAX, OK, Q, REMOVE, UNK,
                            ref_apply)

N = 65
KS = [8, 16, 64]
BAD_ARGS, PENDING = _lib.PAS_GAS_ERR_BAD_ARGS, _lib.PAS_GAS_ANN_PENDING
NODE_NAMES = [f"node-{n}" for n in range(N)]


# ------------------------------------------------------------------ inputs

def card_rows(n_cards, k):
    """The rows of the card-name table: the label cards in sort.Strings order, one parked card
    behind them where the row has room, empty names in the unused slots."""
    rows = []
    for n, nc in enumerate(n_cards):
        label = go_sort_strings([f"card{i}" for i in range(max(int(nc), 0))])
        row = label + ([f"parked{n}"] if len(label) < k else [])
        rows.append(row + [""] * (k - len(row)))
    return rows


def host_route(n_cards, rows, ncont, pods, nodes, anns):
    """What GasCache._plan answers on the host (verdict [E], PENDING for the events it sends)
    and the arrays it sends: cards_per_container [E][C] and ranks [E][ld]."""
    e = len(anns)
    verdict = np.full(e, PENDING, np.int32)
    cpc = np.zeros((e, C), np.int32)
    ranks = []
    for i, ann in enumerate(anns):
        row = []
        if len(ann.split("|")) != ncont[pods[i]]:
            verdict[i] = BAD_ARGS
        elif nodes[i] == -1:
            verdict[i] = OK
        else:
            label = rows[nodes[i]][:max(int(n_cards[nodes[i]]), 0)]
            counts, row = parse_annotation(ann, label)
            if not row:
                verdict[i] = OK
            else:
                cpc[i, :len(counts)] = counts
        ranks.append(row if verdict[i] == PENDING else [])
    ld = max([1] + [len(r) for r in ranks])
    cards = np.full((e, ld), -1, np.int32)
    for i, r in enumerate(ranks):
        cards[i, :len(r)] = r
    return verdict, cpc, cards


@functools.lru_cache(maxsize=None)
def ann_case(k, n_ev=1000, n_live=40, one_node=False):
    """A seeded batch of mixed events as strings, with the host route's verdicts and the oracle's
    answer for the events that reach the walker."""
    import oracle
    rng = np.random.default_rng(7000 + k + n_ev + n_live)
    n_cards = rng.integers(1, k + 1, size=N).astype(np.int32)
    n_cards[0] = k  # a full row: no parked slot
    cap = rng.integers(500, 5000, size=(N, Q)).astype(np.int64)
    used = rng.integers(0, 400, size=(N, k, Q)).astype(np.int64)
    live = rng.choice(N, size=n_live, replace=False)
    if one_node:
        live = live[5:6]
    else:
        n_cards[live[0]] = 0    # no cards label
        n_cards[live[1]] = -1   # a node the lister does not know
    hot = live[2:5]             # usage near INT64_MAX: adds overflow there
    n_cards[hot] = k
    used[hot, 0, 0] = I64_MAX - 500
    used[hot, k - 1, 2] = I64_MAX - 3
    rows = card_rows(n_cards, k)
    n_pods = 64
    req = rng.integers(0, 1000, size=(n_pods, C, Q)).astype(np.int64)
    req[rng.random((n_pods, C, Q)) < 0.1] = 0
    mask = rng.integers(0, 1 << Q, size=(n_pods, C)).astype(np.uint32)
    ncont = rng.integers(1, C + 1, size=n_pods).astype(np.int32)
    ncont[np.arange(n_pods) % 16 == 5] = 0  # a pod without containers is always bad args
    negative = np.arange(n_pods) % 8 == 7   # pods with a negative amount: never on a hot node
    for p in np.nonzero(negative)[0]:
        req[p, rng.integers(0, C), rng.integers(0, Q)] = -int(rng.integers(1, 50))
    mask[np.arange(n_pods) % 16 == 3, 0] |= np.uint32(UNK)  # ADD ignores it, REMOVE does not
    kinds = (rng.random(n_ev) < 0.4).astype(np.int32)  # 1 = REMOVE
    pods = rng.integers(0, n_pods, size=n_ev).astype(np.int32)
    nodes = rng.choice(live, size=n_ev).astype(np.int32)
    on_hot = np.isin(nodes, hot) & negative[pods]
    pods[on_hot] -= 1  # the pod before a negative one is not negative
    anns = []
    for e in range(n_ev):
        names = rows[nodes[e]]
        nc = max(int(n_cards[nodes[e]]), 1)
        segments = []
        for _ in range(int(ncont[pods[e]])):
            listed = [names[r] if rng.random() >= 0.03 else
                      str(rng.choice(["nosuchcard", f"parked{nodes[e]}", "", "card", "card1x"]))
                      for r in rng.integers(0, nc, size=int(rng.integers(0, 5)))]
            segments.append(",".join(listed))
        ann = "|".join(segments)
        dice = rng.random()
        if dice < 0.04:
            ann = ann + "|" if rng.random() < 0.5 else ann.rpartition("|")[0]  # segments off by one
        elif dice < 0.07:
            ann = "|" * (int(ncont[pods[e]]) - 1) if rng.random() < 0.7 else ""  # no card at all
        elif dice < 0.11:
            nodes[e] = -1  # a node the snapshot does not hold
        anns.append(ann)
    verdict, cpc, cards = host_route(n_cards, rows, ncont, pods, nodes, anns)
    pend = np.nonzero(verdict == PENDING)[0]
    want_used, want_pend = ref_apply(oracle, n_cards, used, kinds[pend], pods[pend], nodes[pend],
                                     req, mask, ncont, cpc[pend], cards[pend])
    want_st = verdict.copy()
    want_st[pend] = want_pend
    case = dict(n_cards=n_cards, cap=cap, used=used, kinds=kinds, pods=pods, nodes=nodes, req=req,
                mask=mask, ncont=ncont, verdict=verdict, cpc=cpc, cards=cards, pend=pend,
                want_used=want_used, want_st=want_st)
    for a in case.values():
        a.setflags(write=False)
    case.update(rows=rows, anns=anns, k=k)
    return case


# ------------------------------------------------------------------ CPU: the batches' own reach

@pytest.mark.parametrize("k", KS)
def test_generated_batches_reach_every_outcome(k):
    i = ann_case(k)
    e = len(i["anns"])
    assert e == 1000 and len(np.unique(i["nodes"][i["nodes"] >= 0])) >= 35
    assert len(i["pend"]) >= e // 2                                   # at least half pending
    assert ((i["verdict"] == OK).sum() >= 1 and (i["verdict"] == BAD_ARGS).sum() >= 1)
    assert (i["nodes"] == -1).any() and any(a == "" for a in i["anns"])
    for s in (OK, ERR_INPUT, ERR_OVERFLOW):                           # out of the walker
        assert (i["want_st"][i["pend"]] == s).any(), s
    assert (i["cards"][i["pend"]] == -1).any()                        # unknown cards are listed
    if k >= 16:  # names that are prefixes of each other stand in one row
        assert {"card1", "card10"} <= set(i["rows"][0])


# ------------------------------------------------------------------ GPU plumbing

_gen = [91000]


@pytest.fixture(scope="module")
def ctx2():
    """The second context: the parent's route runs there."""
    c = pas_amd.Context(0)
    yield c
    c.close()


def upload(ctx, i, tables=True):
    _gen[0] += 10
    ctx.gas_snapshot_set(_gen[0], i["n_cards"], i["cap"], i["used"])
    if tables:
        ctx.gas_card_names_set(N, i["k"], *pack_names([c for row in i["rows"] for c in row]))
        ctx.names_set(*pack_names(NODE_NAMES))
    return _gen[0]


def apply_strings(ctx, gen, i, sel=slice(None)):
    anns = [i["anns"][e] for e in np.arange(len(i["anns"]))[sel]]
    return ctx.gas_apply_annotations(gen, gen + 1, i["kinds"][sel], i["pods"][sel],
                                     i["nodes"][sel], i["req"], i["mask"], i["ncont"],
                                     *pack_names(anns))


def parent_route(ctx, gen, i):
    """The statuses of the host route: its own verdicts, pas_gas_apply for the rest."""
    pend = i["pend"]
    st = i["verdict"].copy()
    st[pend] = ctx.gas_apply(gen, gen + 1, i["kinds"][pend], i["pods"][pend], i["nodes"][pend],
                             i["req"], i["mask"], i["ncont"], i["cpc"][pend], i["cards"][pend])
    return st


def check_case(ctx, ctx2, i):
    gen = upload(ctx, i)
    st = apply_strings(ctx, gen, i)
    g, after = ctx.gas_snapshot_get()
    assert g == gen + 1
    gen2 = upload(ctx2, i, tables=False)
    st2 = parent_route(ctx2, gen2, i)
    _, after2 = ctx2.gas_snapshot_get()
    np.testing.assert_array_equal(st, st2)
    np.testing.assert_array_equal(after, after2)
    np.testing.assert_array_equal(st, i["want_st"])       # ... and the oracle underneath
    np.testing.assert_array_equal(after, i["want_used"])


def dev(a):
    import torch
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def dev_blob(names):
    import torch
    off, blob = pack_names(names)
    data = np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)
    return len(blob), dev(off), torch.from_numpy(data.copy()).cuda()


# ------------------------------------------------------------------ resolve parity

def resolve_case(k, n_ev):
    """Five nodes: a full row (L = k), a row whose label is gone (L = 0), a node the lister
    does not know (n_cards -1), a half row with a parked name behind it, and names that differ
    in their last byte only."""
    rng = np.random.default_rng(100 * k + n_ev)
    half = k // 2
    n_cards = np.array([k, 0, -1, half, min(k, 6)], np.int32)
    rows = [go_sort_strings([f"card{i}" for i in range(k)]),
            go_sort_strings([f"card{i}" for i in range(k)]),   # names stand there, L = 0
            [f"card{i}" for i in range(half)] + [""] * (k - half),
            go_sort_strings([f"card{i}" for i in range(half)]) + ["parked"] + [""] * (k - half - 1),
            [f"gpu-{c}" for c in "abcdef"][:min(k, 6)] + [""] * (k - min(k, 6))]
    vocabulary = ["card0", "card1", "card10", "card100", "card", "parked", "gpu-a", "gpu-f",
                  "gpu-", "gpu-aa", "", "é", f"card{k - 1}", f"card{half}"]
    ncont = np.array([1, 2, 3, 0], np.int32)
    pods = rng.integers(0, 4, size=n_ev).astype(np.int32)
    nodes = rng.integers(0, 5, size=n_ev).astype(np.int32)
    anns = []
    for e in range(n_ev):
        segs = int(ncont[pods[e]]) if rng.random() < 0.9 else int(rng.integers(1, 5))
        anns.append("|".join(",".join(rng.choice(vocabulary, size=int(rng.integers(0, 4))))
                             for _ in range(max(segs, 1))))
    nodes[rng.random(n_ev) < 0.05] = -1
    return n_cards, rows, ncont, pods, nodes, anns


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n_ev", [1, 255, 256, 257])  # the 256-lane block edge
def test_resolve_parity(ctx, k, n_ev):
    n_cards, rows, ncont, pods, nodes, anns = resolve_case(k, n_ev)
    _gen[0] += 10
    ctx.gas_snapshot_set(_gen[0], n_cards, np.zeros((5, Q), np.int64),
                         np.zeros((5, k, Q), np.int64))
    ctx.gas_card_names_set(5, k, *pack_names([c for row in rows for c in row]))
    ld = 12
    verdict, listed, cpc, cards = ctx.gas_annotations_resolve(pods, nodes, ncont, C,
                                                              *pack_names(anns), ld)
    seen = set()
    for e, ann in enumerate(anns):
        label = rows[nodes[e]][:max(int(n_cards[nodes[e]]), 0)] if nodes[e] >= 0 else []
        counts, ranks = parse_annotation(ann, label)
        want = (BAD_ARGS if len(counts) != ncont[pods[e]] else OK if nodes[e] == -1 or not ranks
                else PENDING)
        assert verdict[e] == want, (e, ann)
        assert listed[e] == len(ranks)
        assert cpc[e].tolist() == (counts + [0] * C)[:C], (e, ann)
        assert cards[e].tolist() == (ranks + [-1] * ld)[:ld], (e, ann, int(nodes[e]))
        seen.add(want)
    if n_ev > 200:
        assert seen == {BAD_ARGS, OK, PENDING}
        assert (cards >= 0).any() and ctx.gas_snapshot_get()[1].sum() == 0  # nothing resident


@pytest.mark.gpu
def test_resolve_truncates_a_long_list_and_reports_its_length(ctx):
    k = 8
    n_cards, rows, ncont, _, _, _ = resolve_case(k, 1)
    _gen[0] += 10
    ctx.gas_snapshot_set(_gen[0], n_cards, np.zeros((5, Q), np.int64),
                         np.zeros((5, k, Q), np.int64))
    ctx.gas_card_names_set(5, k, *pack_names([c for row in rows for c in row]))
    long = ",".join(f"card{j % k}" if j % 7 else "nosuch" for j in range(200))
    anns = ["card1", long, "card2|card3"]
    verdict, listed, cpc, cards = ctx.gas_annotations_resolve(
        [0, 0, 1], [0, 0, 0], ncont, C, *pack_names(anns), 8)
    assert verdict.tolist() == [PENDING] * 3 and listed.tolist() == [1, 200, 2]
    assert cpc.tolist() == [[1, 0, 0], [200, 0, 0], [1, 1, 0]]
    _, ranks = parse_annotation(long, rows[0])
    assert cards.tolist() == [[1] + [-1] * 7, ranks[:8], [2, 3] + [-1] * 6]


# ------------------------------------------------------------------ apply parity

@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_apply_parity_with_the_host_route_and_the_oracle(ctx, ctx2, k):
    check_case(ctx, ctx2, ann_case(k))


@pytest.mark.gpu
def test_a_batch_across_the_walkers_workgroup(ctx, ctx2):
    i = ann_case(8, 1025, 40)  # 1 025 sorted positions: the walker's second workgroup
    assert len(i["anns"]) == 1025
    check_case(ctx, ctx2, i)


@pytest.mark.gpu
def test_every_event_on_one_node_keeps_the_order(ctx, ctx2, oracle):
    i = ann_case(8, 600, 40, True)
    pend = i["pend"]
    assert len(np.unique(i["nodes"][pend])) == 1 and len(pend) > 300
    # the order matters: the same events with the ADDs first end elsewhere
    order = np.argsort(i["kinds"][pend], kind="stable")
    other, _ = ref_apply(oracle, i["n_cards"], i["used"], i["kinds"][pend][order],
                         i["pods"][pend][order], i["nodes"][pend][order], i["req"], i["mask"],
                         i["ncont"], i["cpc"][pend][order], i["cards"][pend][order])
    assert (other != i["want_used"]).any()
    check_case(ctx, ctx2, i)


@pytest.mark.gpu
def test_one_long_list_among_short_ones_sizes_the_rank_rows(ctx, ctx2):
    base = ann_case(8, 40, 40)
    i = dict(base)
    e = int(np.nonzero((base["nodes"] >= 0) & (base["ncont"][base["pods"]] == 1))[0][0])
    node = int(base["nodes"][e])
    nc = max(int(base["n_cards"][node]), 1)
    anns = list(base["anns"])
    anns[e] = ",".join(base["rows"][node][j % nc] if j % 9 else "nosuch" for j in range(200))
    i["anns"] = anns
    i["verdict"], i["cpc"], i["cards"] = host_route(base["n_cards"], base["rows"], base["ncont"],
                                                    base["pods"], base["nodes"], anns)
    i["pend"] = np.nonzero(i["verdict"] == PENDING)[0]
    assert i["cards"].shape[1] == 200 and e in i["pend"]
    gen = upload(ctx, i)
    st = apply_strings(ctx, gen, i)
    gen2 = upload(ctx2, i, tables=False)
    np.testing.assert_array_equal(st, parent_route(ctx2, gen2, i))
    np.testing.assert_array_equal(ctx.gas_snapshot_get()[1], ctx2.gas_snapshot_get()[1])
    assert (ctx.gas_snapshot_get()[1] != base["used"]).any()


@pytest.mark.gpu
def test_empty_batch_moves_the_generation(ctx):
    i = ann_case(8, 40, 40)
    gen = upload(ctx, i)
    empty = np.zeros(0, np.int32)
    st = ctx.gas_apply_annotations(gen, gen + 1, empty, empty, empty, i["req"], i["mask"],
                                   i["ncont"], [0], b"")
    assert len(st) == 0 and ctx.gas_snapshot_get()[0] == gen + 1
    st = ctx.gas_apply_annotations_names(gen + 1, gen + 2, empty, empty, [0], b"", i["req"],
                                         i["mask"], i["ncont"], [0], b"")
    assert len(st) == 0 and ctx.gas_snapshot_get()[0] == gen + 2
    np.testing.assert_array_equal(ctx.gas_snapshot_get()[1], i["used"])


# ------------------------------------------------------------------ the forms agree

def node_name(n):
    return NODE_NAMES[n] if n >= 0 else "a-node-nobody-holds"


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_names_form_and_device_forms_agree_with_the_slot_form(ctx, k):
    import torch
    i = ann_case(k)
    e = len(i["anns"])
    names = [node_name(n) for n in i["nodes"]]
    gen = upload(ctx, i)
    st = ctx.gas_apply_annotations_names(gen, gen + 1, i["kinds"], i["pods"], *pack_names(names),
                                         i["req"], i["mask"], i["ncont"], *pack_names(i["anns"]))
    np.testing.assert_array_equal(st, i["want_st"])
    np.testing.assert_array_equal(ctx.gas_snapshot_get()[1], i["want_used"])
    assert ctx.names_info()[:2] == (N, N)  # lookup only: the unknown name took no slot
    # the _device forms on torch tensors
    stream = torch.cuda.current_stream()
    n_ann, ann_off, ann_bytes = dev_blob(i["anns"])
    pods_t = {name: dev(i[name]) for name in ("kinds", "pods", "nodes", "req", "mask", "ncont")}
    for by_name in (False, True):
        gen = upload(ctx, i)
        st_t = torch.full((e,), -7, dtype=torch.int32, device="cuda")
        if by_name:
            n_nm, nm_off, nm_bytes = dev_blob(names)
            ctx.gas_apply_annotations_names_device(
                gen, gen + 1, e, pods_t["kinds"], pods_t["pods"], n_nm, nm_off, nm_bytes,
                i["req"].shape[0], C, pods_t["req"], pods_t["mask"], pods_t["ncont"], n_ann,
                ann_off, ann_bytes, st_t, stream=stream)
        else:
            ctx.gas_apply_annotations_device(
                gen, gen + 1, e, pods_t["kinds"], pods_t["pods"], pods_t["nodes"],
                i["req"].shape[0], C, pods_t["req"], pods_t["mask"], pods_t["ncont"], n_ann,
                ann_off, ann_bytes, st_t, stream=stream)
        stream.synchronize()
        g, after = ctx.gas_snapshot_get()
        assert g == gen + 1
        np.testing.assert_array_equal(st_t.cpu().numpy(), i["want_st"])
        np.testing.assert_array_equal(after, i["want_used"])


@pytest.mark.gpu
def test_unknown_and_empty_node_names(ctx):
    i = ann_case(8, 40, 40)
    gen = upload(ctx, i)
    e = int(np.nonzero(i["verdict"] == PENDING)[0][0])
    one = dict(kinds=i["kinds"][e:e + 1].repeat(3), pods=i["pods"][e:e + 1].repeat(3))
    names = ["a-node-nobody-holds", "", NODE_NAMES[int(i["nodes"][e])]]
    st = ctx.gas_apply_annotations_names(gen, gen + 1, one["kinds"], one["pods"],
                                         *pack_names(names), i["req"], i["mask"], i["ncont"],
                                         *pack_names([i["anns"][e]] * 3))
    assert st[:2].tolist() == [OK, BAD_ARGS] and st[2] == i["want_st"][e]
    g, after = ctx.gas_snapshot_get()
    assert g == gen + 1
    changed = np.nonzero((after != i["used"]).reshape(N, -1).any(axis=1))[0]
    assert set(changed) <= {int(i["nodes"][e])}  # the first two changed nothing


# ------------------------------------------------------------------ malformed device arrays

def malformed_case(oracle, k):
    """Events whose arrays a host form would refuse, with what the rules make of them."""
    base = ann_case(k, 40, 40)
    node = int(np.nonzero((base["n_cards"] >= 2) & (base["used"].max(axis=(1, 2)) < 10**6))[0][0])
    n_pods = 5
    req = np.zeros((n_pods, C, Q), np.int64)
    req[:, :, :] = np.arange(1, Q + 1) * 10
    mask = np.full((n_pods, C), 7, np.uint32)
    ncont = np.array([1, 2, C + 5, -3, 2**31 - 1], np.int32)  # 2.. are out of range
    blob = b"card0|card1,card0|card1xcard0"
    n_b = len(blob)
    # event: kind, pod, node, span (begin, end), the status the rules give
    rows = [
        (ADD, 0, node, (0, 5), OK),                    # 0 "card0": valid
        (ADD, 1, node, (0, 17), OK),                   # 1 "card0|card1,card0": valid
        (7, 0, node, (0, 5), ERR_INPUT),               # 2 a kind of 7
        (-1, 0, node, (0, 5), ERR_INPUT),              # 3
        (ADD, n_pods, node, (0, 5), ERR_INPUT),        # 4 pod out of range
        (ADD, 0, N + 5, (0, 5), ERR_INPUT),            # 5 a node of n_nodes + 5
        (ADD, 0, -2**31, (0, 5), ERR_INPUT),           # 6
        (ADD, 0, -1, (0, 5), OK),                      # 7 node -1: settled, nothing changes
        (ADD, 0, node, (11, 5), OK),                   # 8 decreasing: the empty annotation
        (ADD, 0, node, (-40, 5), OK),                  # 9 begin clamped to 0: "card0"
        (ADD, 0, node, (24, n_b + 900), OK),           # 10 end clamped to n_bytes: "card0"
        (ADD, 0, node, (n_b + 7, n_b + 900), OK),      # 11 both past the blob: empty
        (REMOVE, 0, node, (2**62, -2**62), OK),        # 12 far out both ways: empty
        (ADD, 2, node, (0, n_b), OK),                  # 13 n_containers C + 5 reads as C = 3
        (ADD, 3, node, (0, 5), BAD_ARGS),              # 14 n_containers -3 reads as 0
        (ADD, 4, node, (0, 17), BAD_ARGS),             # 15 INT32_MAX reads as C: 2 segments
        (ADD, 0, node, (0, 17), BAD_ARGS),             # 16 2 segments, 1 container
    ]
    e = len(rows)
    kinds = np.array([r[0] for r in rows], np.int32)
    pods = np.array([r[1] for r in rows], np.int32)
    nodes = np.array([r[2] for r in rows], np.int32)
    # every event has its own pair of offsets: off[e] and off[e + 1] must serve two events, so
    # the events alternate with filler events (pod out of range) that absorb the other end
    off = np.zeros(2 * e + 1, np.int64)
    for j, r in enumerate(rows):
        off[2 * j], off[2 * j + 1] = r[4 - 1]
    kinds2 = np.full(2 * e, ADD, np.int32)
    pods2 = np.full(2 * e, -1, np.int32)       # the fillers: PAS_GAS_ERR_INPUT
    nodes2 = np.full(2 * e, node, np.int32)
    kinds2[0::2], pods2[0::2], nodes2[0::2] = kinds, pods, nodes
    want = np.full(2 * e, ERR_INPUT, np.int32)
    want[0::2] = [r[4] for r in rows]
    # what the valid events do: ADDs of pods 0, 1, 2 as parse_annotation reads their spans
    label = base["rows"][node][:int(base["n_cards"][node])]
    texts = {0: "card0", 1: "card0|card1,card0", 9: "card0", 10: "card0",
             13: "card0|card1,card0|card1xcard0"}
    ncont_read = np.clip(ncont.astype(np.int64), 0, C).astype(np.int32)
    cpc = np.zeros((len(texts), C), np.int32)
    cards = np.full((len(texts), 4), -1, np.int32)
    for j, (ev, text) in enumerate(texts.items()):
        counts, ranks = parse_annotation(text, label)
        cpc[j, :len(counts)], cards[j, :len(ranks)] = counts, ranks
    ev = list(texts)
    want_used, want_st = ref_apply(oracle, base["n_cards"], base["used"], kinds[ev], pods[ev],
                                   nodes[ev], req, mask, ncont_read, cpc, cards)
    assert (want_st == OK).all() and (want_used != base["used"]).any()
    return dict(base=base, e=e, n_pods=n_pods, n_b=n_b, blob=blob, kinds2=kinds2, pods2=pods2,
                nodes2=nodes2, req=req, mask=mask, ncont=ncont, off=off, want=want,
                want_used=want_used, texts=texts)


def test_malformed_case_is_what_it_says(oracle):
    # no GPU: the valid events of the malformed batch change the usage and all succeed
    for k in KS:
        m = malformed_case(oracle, k)
        assert (m["want"][0::2] == OK).sum() == 9 and (m["want"][1::2] == ERR_INPUT).all()
        assert m["blob"][24:] == b"card0" and m["n_b"] == 29


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_device_form_with_malformed_arrays(ctx, oracle, k):
    # nothing here is meant to fault: the _device form clamps and settles
    import torch
    m = malformed_case(oracle, k)
    base, e, n_pods, n_b, blob, texts = (m[x] for x in ("base", "e", "n_pods", "n_b", "blob",
                                                        "texts"))
    kinds2, pods2, nodes2, req, mask, ncont, off, want, want_used = (
        m[x] for x in ("kinds2", "pods2", "nodes2", "req", "mask", "ncont", "off", "want",
                       "want_used"))
    gen = upload(ctx, base)
    guard = 64
    st_buf = torch.full((2 * e + 2 * guard,), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    ctx.gas_apply_annotations_device(
        gen, gen + 1, 2 * e, dev(kinds2), dev(pods2), dev(nodes2), n_pods, C, dev(req), dev(mask),
        dev(ncont), n_b, dev(off), torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda(),
        st_buf[guard:guard + 2 * e], stream=stream)
    stream.synchronize()
    got = st_buf.cpu().numpy()
    assert (got[:guard] == -7).all() and (got[guard + 2 * e:] == -7).all()
    np.testing.assert_array_equal(got[guard:guard + 2 * e], want)
    g, after = ctx.gas_snapshot_get()
    assert g == gen + 1
    np.testing.assert_array_equal(after, want_used)  # usage unchanged for every failed event
    # the resolve form on the same arrays: guard words around all four outputs
    ld = 3
    outs = [torch.full((w * 2 * e + 2 * guard,), -7, dtype=torch.int32, device="cuda")
            for w in (1, 1, C, ld)]
    views = [o[guard:o.numel() - guard] for o in outs]
    ctx.gas_annotations_resolve_device(
        2 * e, dev(pods2), dev(nodes2), n_pods, dev(ncont), C, n_b, dev(off),
        torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda(), ld, *views, stream=stream)
    stream.synchronize()
    for o in outs:
        o = o.cpu().numpy()
        assert (o[:guard] == -7).all() and (o[-guard:] == -7).all()
        assert (o[guard:-guard] != -7).all()  # every word of the outputs is written
    verdict = outs[0].cpu().numpy()[guard:-guard]
    pending = np.isin(np.arange(2 * e), [2 * x for x in list(texts) + [2, 3]])  # (no kinds here)
    np.testing.assert_array_equal(verdict == PENDING, pending)
    # the host form refuses the same arrays before anything runs
    for j in (2, 4, 5, 6, 8, 9, 13, 14):
        sl = slice(2 * j, 2 * j + 1)
        with pytest.raises(pas_amd.PasError) as err:
            ctx.gas_apply_annotations(gen + 1, gen + 2, kinds2[sl], pods2[sl], nodes2[sl], req,
                                      mask, ncont, off[2 * j:2 * j + 2], blob)
        assert err.value.code == _lib.PAS_EINVAL, j
    g, still = ctx.gas_snapshot_get()
    assert g == gen + 1
    np.testing.assert_array_equal(still, after)


# ------------------------------------------------------------------ return codes

@pytest.mark.gpu
def test_return_codes_and_generation(ctx):
    i = ann_case(8, 40, 40)
    gen = upload(ctx, i)

    def code(call, *args):
        with pytest.raises(pas_amd.PasError) as err:
            call(*args)
        return err.value.code

    assert code(apply_strings, ctx, gen - 1, i) == _lib.PAS_ESTALE     # a wrong gen_from
    g, after = ctx.gas_snapshot_get()
    assert g == gen
    np.testing.assert_array_equal(after, i["used"])
    # a card-name table of another shape: PAS_EINVAL, the message names it
    ctx.gas_card_names_resize(N + 1, 8)
    assert code(apply_strings, ctx, gen, i) == _lib.PAS_EINVAL
    assert "card-name table" in ctx.last_error()
    ctx.gas_card_names_set(N, 16, *pack_names([""] * (N * 16)))
    assert code(apply_strings, ctx, gen, i) == _lib.PAS_EINVAL
    # without a card-name table, and the names form without a name table: PAS_ENOSNAP
    ctx.gas_card_names_drop()
    assert code(apply_strings, ctx, gen, i) == _lib.PAS_ENOSNAP
    assert code(ctx.gas_annotations_resolve, i["pods"], i["nodes"], i["ncont"], C,
                *pack_names(i["anns"]), 4) == _lib.PAS_ENOSNAP
    upload(ctx, i)
    gen = _gen[0]
    ctx.names_drop()
    names = pack_names([node_name(n) for n in i["nodes"]])
    assert code(ctx.gas_apply_annotations_names, gen, gen + 1, i["kinds"], i["pods"], *names,
                i["req"], i["mask"], i["ncont"], *pack_names(i["anns"])) == _lib.PAS_ENOSNAP
    g, after = ctx.gas_snapshot_get()
    assert g == gen
    np.testing.assert_array_equal(after, i["used"])
    # the generation moves when nothing was pending
    settled = np.nonzero(i["verdict"] != PENDING)[0]
    assert len(settled) >= 2
    st = apply_strings(ctx, gen, i, settled)
    np.testing.assert_array_equal(st, i["verdict"][settled])
    g, after = ctx.gas_snapshot_get()
    assert g == gen + 1
    np.testing.assert_array_equal(after, i["used"])


# ------------------------------------------------------------------ end to end: the cache

KINDS = ["gpu.intel.com/i915", "gpu.intel.com/memory.max"]


def run_script(ctx, device_events, seed=2024, n_items=200):
    """One seeded script of mixed pod and node items through a GasCache over `ctx`; after every
    flush a record of (outcomes, annotated, card_names, parked, usage)."""
    from pas_amd.gas_cache import GasCache
    from test_gas_cache_nodes import node_obj, pod_obj
    rng = np.random.default_rng(seed)
    labels = {f"n{j}": [f"card{c}" for c in range(int(rng.integers(1, 5)))] for j in range(6)}
    gc = GasCache.from_nodes(ctx, 500 + 1000 * int(device_events),
                             [node_obj(n, cards) for n, cards in labels.items()], KINDS,
                             spare_nodes=1, device_events=device_events)
    records, pods, fresh = [], {}, [0]

    def snap(outcomes):
        records.append((outcomes, dict(gc.annotated), [list(c) for c in gc.card_names],
                        [list(p) for p in gc.parked], ctx.gas_snapshot_get()[1].copy()))

    for item in range(n_items):
        dice = rng.random()
        node = str(rng.choice(list(labels)))
        if dice < 0.45 or not pods:                               # pod add / update
            name = f"p{fresh[0]}"
            fresh[0] += 1
            nc = int(rng.integers(1, 3))
            cards = labels[node] or ["card0"]
            ann = "|".join(",".join(rng.choice(cards + ["ghostcard"],
                                               size=int(rng.integers(0, 3))))
                           for _ in range(nc if rng.random() > 0.1 else nc + 1))
            target = node if rng.random() > 0.08 else str(rng.choice(["", "nowhere"]))
            pods[name] = pod_obj(name, target, [(int(rng.integers(1, 3)), 100)] * nc, ann)
            (gc.add_pod if rng.random() < 0.5 else
             lambda p: gc.update_pod(None, p))(pods[name])
        elif dice < 0.6:                                          # complete
            name = str(rng.choice(list(pods)))
            done = dict(pods[name], status={"phase": "Succeeded"})
            gc.update_pod(None, done)
        elif dice < 0.7:                                          # delete (the quirk)
            name = str(rng.choice(list(pods)))
            gc.delete_pod(pods.pop(name))
        elif dice < 0.85:                                         # cards leave and return
            keep = [c for c in [f"card{c}" for c in range(6)] if rng.random() < 0.5]
            labels[node] = keep
            gc.update_node(None, node_obj(node, keep or None))
        elif dice < 0.9:                                          # node delete, then back later
            gc.delete_node(node_obj(node, None))
            labels[node] = []
        else:
            labels[node] = [f"card{c}" for c in range(int(rng.integers(1, 4)))]
            gc.add_node(node_obj(node, labels[node]))
        if item == 60:                                            # one growth: nodes and cards
            for j in range(2):
                labels[f"big{j}"] = [f"card{c}" for c in range(9 + j)]
                gc.add_node(node_obj(f"big{j}", labels[f"big{j}"]))
        if item % 7 == 6:
            snap(gc.flush())
        if item == 120:
            snap(gc.flush())
            snap(("compact", gc.compact(spare_nodes=1)))
        if item == 160:
            snap(gc.flush())
            snap(("rebuild", gc.rebuild(list(pods.values()))))
    snap(gc.flush())
    return records, gc


@pytest.mark.gpu
def test_cache_with_device_events_reproduces_the_default_mode(ctx, ctx2):
    want, plain = run_script(ctx2, False)
    got, dev_gc = run_script(ctx, True)
    assert len(want) == len(got) > 25
    for step, (w, g) in enumerate(zip(want, got)):
        assert w[0] == g[0], step          # flush() outcomes, item by item
        assert w[1:4] == g[1:4], step      # annotated, card_names, parked
        np.testing.assert_array_equal(w[4], g[4], err_msg=f"usage after step {step}")
    outcomes = [o[2] for w in want if isinstance(w[0], list) for o in w[0]]
    for kind in ("ok", "skipped", "bad_args", "input"):
        assert kind in outcomes, kind
    assert len(plain.node_names) == len(dev_gc.node_names) and dev_gc.max_cards == 16
    # the device tables are the cache's
    k = dev_gc.max_cards
    off, blob = ctx.gas_card_names_get()
    names = [blob[off[j]:off[j + 1]].decode() for j in range(len(off) - 1)]
    for slot in range(len(dev_gc.node_names)):
        row = dev_gc.card_names[slot] + dev_gc.parked[slot]
        assert names[slot * k:(slot + 1) * k] == row + [""] * (k - len(row)), slot
    off, blob = ctx.names_get()
    assert [blob[off[j]:off[j + 1]].decode() or None for j in range(len(off) - 1)] == \
        dev_gc.node_names
