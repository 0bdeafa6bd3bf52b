"""The extender verbs for a batch of requests in request terms: pas_tas_prioritize_requests,
pas_tas_filter_requests and pas_gas_fit_requests (and their _device forms) against the oracle
called once per request.  One batch mixes the lengths at which the kernels change path: empty,
one position, either side of a wave (64) and of a workgroup (256), and either side of S, the
longest request the batched prioritize sorts in LDS (S + 1 takes the single-request path inside
the batch)."""
import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from helpers import pack_bits, unpack_bits, w64
from oracle import RULE_DTYPE

S = 2048  # csrc/request_batch.h kRequestCap
I32_MAX = 2**31 - 1
N, M = 3000, 4
WIDE = 3
SCALE = [3, 0, 7, 3]
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1]
_gen = [70_000]


def test_lib_declares_the_six_functions():
    for fam in ("pas_tas_prioritize_requests", "pas_tas_filter_requests", "pas_gas_fit_requests"):
        assert fam in _lib.SIGNATURES and fam + "_device" in _lib.SIGNATURES
        # the _device form takes the same arguments plus what the host form cannot know
        assert len(_lib.SIGNATURES[fam + "_device"][1]) > len(_lib.SIGNATURES[fam][1])


# ------------------------------------------------------------------------- requests

def make_request(rng, n_nodes, n, dup=0.1, unknown=0.05):
    """n request positions over n_nodes snapshot nodes: mostly distinct, about 10 % repeats of
    an earlier position's node (one pair more than 64 and one more than 256 positions apart
    when the request is long enough), about 5 % ids the snapshot does not hold."""
    req = rng.permutation(max(n_nodes, 1))[np.arange(n) % max(n_nodes, 1)].astype(np.int32)
    for j in np.nonzero(rng.random(n) < dup)[0]:
        if j:
            req[j] = req[rng.integers(0, j)]
    req[rng.random(n) < unknown] = rng.choice([-1, n_nodes, I32_MAX, -7, n_nodes + 5])
    if n > 70:
        req[2] = abs(int(req[2])) % n_nodes
        req[70] = req[2]
    if n > 300:
        req[0] = abs(int(req[0])) % n_nodes
        req[n - 1] = req[0]
    if n > 3:
        req[1], req[3] = -1, n_nodes
    if n > 5:
        req[5] = I32_MAX
    return req


def make_requests(rng, n_nodes, lengths):
    """The length mix, one request of unknown ids only, and two requests that list the same
    nodes in different orders.  Returns (req_off, req_node, [request arrays])."""
    reqs = [make_request(rng, n_nodes, n) for n in lengths]
    reqs.append(rng.choice([-1, n_nodes, I32_MAX], 100).astype(np.int32))
    same = make_request(rng, n_nodes, 200)
    reqs += [same, same[::-1].copy()]
    off = np.concatenate([[0], np.cumsum([len(r) for r in reqs])]).astype(np.int32)
    return off, np.concatenate(reqs).astype(np.int32), reqs


def gather_bits(node_bits, req, unknown_value):
    """Per-node verdicts [n_nodes] bool gathered to request positions."""
    req = np.asarray(req, np.int64)
    known = (req >= 0) & (req < len(node_bits))
    out = np.full(len(req), unknown_value, bool)
    out[known] = node_bits[req[known]]
    return out


# ------------------------------------------------------------------------- TAS snapshot

class Tas:
    pass


@pytest.fixture(scope="module")
def tas(ctx):
    """N x 4 columns, about 20 % of the nodes absent from each: column 0 milli with few
    distinct values (and int64-range outliers), column 1 at scale 0, column 2 at scale 7,
    column 3 wide.  t.u / t.s are the oracle's per-value decimal form of the same values."""
    rng = np.random.default_rng(0xBA7C)
    t = Tas()
    k = rng.integers(0, 5, (M, N)).astype(np.int64)
    v = np.zeros((M, N), np.int64)
    v[0] = k[0] * 1000
    v[0, ::97] = rng.integers(-2**62, 2**62, len(range(0, N, 97)))
    v[1] = k[1]
    v[2] = k[2] * 10**7 + rng.integers(0, 2, N)
    whole = rng.choice(np.arange(-3, 4), N).astype(np.int64)
    nano = rng.choice(np.array([0, 0, 1, 500_000_000, 999_999_999], np.uint32), N)
    big = rng.random(N) < 0.2
    whole[big] = rng.choice(rng.integers(-2**62, 2**62, 6), int(big.sum()))
    nano[big] = 0
    pres_b = rng.random((M, N)) >= 0.2
    t.pres = pack_bits(pres_b)
    t.pres_b = pres_b
    t.u = v.copy()
    t.s = np.repeat(np.array(SCALE, np.int8)[:, None], N, axis=1)
    frac = nano != 0
    t.u[WIDE] = np.where(frac, whole * 10**9 + nano.astype(np.int64), whole)
    t.s[WIDE] = np.where(frac, 9, 0)
    _gen[0] += 2
    ctx.tas_snapshot_set(_gen[0] - 1, v, t.pres, SCALE)
    ctx.tas_snapshot_update_wide(_gen[0] - 1, _gen[0], [WIDE], whole[None], nano[None],
                                 t.pres[WIDE:WIDE + 1])
    assert ctx.tas_snapshot_wide_count() == 1
    t.gen = _gen[0]
    t.off, t.req, t.reqs = make_requests(rng, N, LENGTHS)
    # per request another metric and another operator, among them an unknown one (3); one
    # request without a scheduling rule (metric -1)
    R = len(t.reqs)
    t.prio = np.zeros(R, RULE_DTYPE)
    for r in range(R):
        t.prio[r] = (r % M, (r + r // M) % 4, 0)
    t.prio[4]["metric"] = -1
    return t


def want_prioritize(oracle, t, r):
    return oracle.prioritize_request(t.u, t.pres, t.prio[r], t.reqs[r], v_scale=t.s)


def check_lists(oracle, t, pos, lens):
    for r, req in enumerate(t.reqs):
        want = want_prioritize(oracle, t, r)
        o = t.off[r]
        assert lens[r] == len(want), f"request {r} (n {len(req)})"
        np.testing.assert_array_equal(pos[o: o + lens[r]], want, err_msg=f"request {r}")
        assert (pos[o + lens[r]: t.off[r + 1]] == -1).all(), f"request {r}: tail"


# ------------------------------------------------------------------------- prioritize

@pytest.mark.gpu
def test_prioritize_batch_matches_oracle_per_request(ctx, oracle, tas):
    t = tas
    assert {len(r) for r in t.reqs} >= set(LENGTHS)
    assert {int(m) for m in t.prio["metric"]} == {-1, 0, 1, 2, 3}
    assert {int(o) for o in t.prio["op"]} == {0, 1, 2, 3}
    pos, lens = ctx.tas_prioritize_requests(t.gen, t.off, t.prio, t.req)
    check_lists(oracle, t, pos, lens)
    # the cases are in the batch: ties decided by position, a wide column in both directions,
    # an empty list for metric -1 and for the all-unknown request, the same nodes in two orders
    assert lens[4] == 0 and lens[len(LENGTHS)] == 0
    a, b = len(t.reqs) - 2, len(t.reqs) - 1
    assert lens[a] > 100 and lens[b] > 100
    wide_ops = {int(t.prio[r]["op"]) for r in range(len(t.reqs)) if t.prio[r]["metric"] == WIDE}
    assert {0, 1} <= wide_ops


@pytest.mark.gpu
def test_prioritize_batch_same_rule_every_operator(ctx, oracle, tas):
    # every (metric, operator) over the whole length mix, so each length meets each column kind
    t = tas
    for m in range(M):
        for op in (0, 1):
            prio = np.zeros(len(t.reqs), RULE_DTYPE)
            prio[:] = (m, op, 0)
            pos, lens = ctx.tas_prioritize_requests(t.gen, t.off, prio, t.req)
            for r, req in enumerate(t.reqs):
                want = oracle.prioritize_request(t.u, t.pres, prio[r], req, v_scale=t.s)
                got = pos[t.off[r]: t.off[r] + lens[r]]
                np.testing.assert_array_equal(got, want, err_msg=f"metric {m} op {op} req {r}")


@pytest.mark.gpu
def test_prioritize_batch_of_one_equals_single_call(ctx, tas):
    t = tas
    for r in (1, 3, 6, 8, 9, 10, len(t.reqs) - 1):
        one = ctx.tas_prioritize_request(t.gen, t.prio[r], t.reqs[r])
        pos, lens = ctx.tas_prioritize_requests(t.gen, [0, len(t.reqs[r])], t.prio[r: r + 1],
                                                t.reqs[r])
        np.testing.assert_array_equal(pos[: lens[0]], one, err_msg=f"request {r}")
        assert (pos[lens[0]:] == -1).all()


@pytest.mark.gpu
def test_prioritize_device_form_equals_host_form(ctx, tas):
    import torch
    t = tas
    pos, lens = ctx.tas_prioritize_requests(t.gen, t.off, t.prio, t.req)
    req_t = torch.from_numpy(t.req).cuda()
    pos_t = torch.full((len(t.req),), 77, dtype=torch.int32, device="cuda")
    len_t = torch.full((len(t.reqs),), 77, dtype=torch.int32, device="cuda")
    ctx.tas_prioritize_requests_device(t.gen, t.off, t.prio, req_t, pos_t, len_t,
                                       stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(len_t.cpu().numpy(), lens)
    np.testing.assert_array_equal(pos_t.cpu().numpy(), pos)


@pytest.mark.gpu
def test_prioritize_errors_and_empty_batches(ctx, tas):
    t = tas
    pos, lens = ctx.tas_prioritize_requests(t.gen, [0], np.zeros(0, RULE_DTYPE),
                                            np.zeros(0, np.int32))
    assert len(pos) == 0 and len(lens) == 0
    pos, lens = ctx.tas_prioritize_requests(t.gen, [0, 0, 0], t.prio[:2], np.zeros(0, np.int32))
    assert len(pos) == 0 and list(lens) == [0, 0]
    bad = t.prio.copy()
    bad[2]["metric"] = M
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_prioritize_requests(t.gen, t.off, bad, t.req)
    assert e.value.code == _lib.PAS_EINVAL
    off = t.off.copy()
    off[3], off[4] = off[4], off[3]
    assert off[4] < off[3]
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_prioritize_requests(t.gen, off, t.prio, t.req)
    assert e.value.code == _lib.PAS_EINVAL
    off = t.off.copy()
    off[0] = 1
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_prioritize_requests(t.gen, off, t.prio, t.req)
    assert e.value.code == _lib.PAS_EINVAL
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_prioritize_requests(t.gen + 1, t.off, t.prio, t.req)
    assert e.value.code == _lib.PAS_ESTALE


# ------------------------------------------------------------------------- filter

def make_filter_rules(rng, n_requests):
    """0, 1 and 16 rules per request in turn; the lists of 16 start with a rule on a column
    the snapshot lacks and a rule on the wide column."""
    rules, off = [], [0]
    for r in range(n_requests):
        n = (0, 1, 16)[r % 3]
        rs = np.zeros(n, RULE_DTYPE)
        rs["metric"] = rng.choice([-1, -1, 0, 1, 2, WIDE], n)
        rs["op"] = rng.integers(0, 3, n)
        rs["target"] = rng.choice([0, 1, 2, 3, 4, 9, 9, 9, -9], n)
        if n == 16:
            rs[0] = (-1, 1, 0)
            rs[1] = (WIDE, int(rng.integers(0, 3)), int(rng.integers(-2, 3)))
            rs[2] = (M + 3, 0, 5)  # past the snapshot's columns: not cached either
        rules.append(rs)
        off.append(off[-1] + n)
    return np.concatenate(rules), np.array(off, np.int32)


def want_filter_rows(oracle, t, rules, rule_off):
    R = len(t.reqs)
    none = np.zeros(R, RULE_DTYPE)
    none["metric"] = -1
    ok, _, _ = oracle.tas_eval(t.u, t.pres, rules, rule_off, none, flags=1, v_scale=t.s)
    ok = unpack_bits(ok, N)
    return [gather_bits(ok[r], req, True) for r, req in enumerate(t.reqs)]


def check_rows(rows, reqs, want, fill=None, what=""):
    """Row r: the wanted bits, zeros up to the end of the request's last word, and (fill
    given) the pre-filled pattern in every word after it."""
    for r, req in enumerate(reqs):
        n, words = len(req), w64(len(req))
        got = unpack_bits(rows[r, :words], words * 64) if words else np.zeros(0, bool)
        np.testing.assert_array_equal(got[:n], want[r], err_msg=f"{what} request {r}")
        assert not got[n:].any(), f"{what} request {r}: bits past the request"
        if fill is not None:
            assert (rows[r, words:] == fill).all(), f"{what} request {r}: words past the row"


@pytest.fixture(scope="module")
def filt(oracle, tas):
    rng = np.random.default_rng(0xF117)
    f = Tas()
    f.rules, f.rule_off = make_filter_rules(rng, len(tas.reqs))
    f.want = want_filter_rows(oracle, tas, f.rules, f.rule_off)
    return f


@pytest.mark.gpu
def test_filter_batch_matches_oracle_gathered_to_positions(ctx, tas, filt):
    t, f = tas, filt
    allw = np.concatenate(f.want)
    known = np.concatenate([(r >= 0) & (r < N) for r in t.reqs])
    assert 0.05 < allw[known].mean() < 0.95 and allw[~known].all()
    fill = np.uint64(0xA5A5A5A5A5A5A5A5)
    ld = w64(S + 1) + 3
    out = np.full((len(t.reqs), ld), fill, np.uint64)
    rows = ctx.tas_filter_requests(t.gen, t.off, f.rules, f.rule_off, t.req, out=out)
    check_rows(rows, t.reqs, f.want, fill, "host")
    # the tightest pitch
    rows = ctx.tas_filter_requests(t.gen, t.off, f.rules, f.rule_off, t.req)
    assert rows.shape[1] == w64(S + 1)
    check_rows(rows, t.reqs, f.want, None, "tight")
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_filter_requests(t.gen, t.off, f.rules, f.rule_off, t.req,
                                out=np.zeros((len(t.reqs), w64(S + 1) - 1), np.uint64))
    assert e.value.code == _lib.PAS_EINVAL
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_filter_requests(t.gen + 1, t.off, f.rules, f.rule_off, t.req)
    assert e.value.code == _lib.PAS_ESTALE


def _rules_t(rules):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rules).view(np.int64).copy()).cuda()


def filter_device(ctx, t, rules, d_rule_off, ld, fill):
    import torch
    out_t = torch.from_numpy(np.full((len(t.reqs), ld), fill, np.uint64).view(np.int64)).cuda()
    ctx.tas_filter_requests_device(t.gen, t.off, len(rules), _rules_t(rules),
                                   torch.from_numpy(np.asarray(d_rule_off, np.int32)).cuda(),
                                   torch.from_numpy(t.req).cuda(), out_t, ld,
                                   stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out_t.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
def test_filter_device_form_equals_host_form(ctx, tas, filt):
    t, f = tas, filt
    fill = np.uint64(0x0123456789ABCDEF)
    rows = filter_device(ctx, t, f.rules, f.rule_off, w64(S + 1) + 1, fill)
    check_rows(rows, t.reqs, f.want, fill, "device")


@pytest.mark.gpu
def test_filter_unknown_operator(ctx, oracle, tas, filt):
    # on a cached column with nodes: the reference's panic in the host form, skipped in the
    # _device form (as pas_tas_eval / pas_tas_eval_device)
    t, f = tas, filt
    rules = f.rules.copy()
    bad = int(f.rule_off[1])  # request 1's only rule
    rules[bad] = (0, 3, 1)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.tas_filter_requests(t.gen, t.off, rules, f.rule_off, t.req)
    assert e.value.code == _lib.PAS_EINVAL and "unknown operator" in str(e.value)
    skipped = rules.copy()
    skipped[bad]["metric"] = -1  # the same batch with the rule never evaluated
    skipped[bad]["op"] = 0
    want = want_filter_rows(oracle, t, skipped, f.rule_off)
    rows = filter_device(ctx, t, rules, f.rule_off, w64(S + 1), np.uint64(0))
    check_rows(rows, t.reqs, want, None, "device, unknown operator")
    # never evaluated (column not cached): not an error in the host form either
    rules[bad] = (-1, 3, 1)
    check_rows(ctx.tas_filter_requests(t.gen, t.off, rules, f.rule_off, t.req), t.reqs, want,
               None, "host, unknown operator on a missing column")


@pytest.mark.gpu
def test_filter_device_rule_offsets_that_are_no_csr(ctx, oracle, tas, filt):
    # read clamped into [0, n_rules] and non-decreasing per request (pas_tas_eval_device's
    # contract): the result is that of the clamped spans, and nothing outside the arrays is read
    t, f = tas, filt
    rng = np.random.default_rng(5)
    n_rules, R = len(f.rules), len(t.reqs)
    raw = rng.integers(-5, n_rules + 6, R + 1).astype(np.int32)
    raw[3], raw[4] = n_rules + 1000, -1000
    spans, off = [], [0]
    for r in range(R):
        a = min(max(int(raw[r]), 0), n_rules)
        b = min(max(int(raw[r + 1]), a), n_rules)
        spans.append(f.rules[a:b])
        off.append(off[-1] + b - a)
    want = want_filter_rows(oracle, t, np.concatenate(spans), np.array(off, np.int32))
    rows = filter_device(ctx, t, f.rules, raw, w64(S + 1), np.uint64(0))
    check_rows(rows, t.reqs, want, None, "device, clamped spans")


# ------------------------------------------------------------------------- GAS

GAS_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 300]
UNKNOWN_KIND = 0x80000000


def gas_case(rng, n, k, q=3, c=4):
    """n nodes of up to k cards (among them n_cards -1 and 0) whose cards take up to 300
    selections each, and one pod per request: 1 to 4 containers; 0, 1, 3 and more than 64
    selections; one pod with a kind the snapshot lacks beside an i915 request."""
    n_cards = rng.integers(-1, k + 1, n).astype(np.int32)
    n_cards[rng.random(n) < 0.5] = k
    n_cards[0], n_cards[1] = -1, 0
    cap = rng.integers(2_000, 200_000, (n, q)).astype(np.int64)
    cap[:, 0] = rng.integers(1, 301, n)
    used = rng.integers(0, 2_000, (n, k, q)).astype(np.int64)
    used[:, :, 0] = rng.integers(0, 150, (n, k))
    off, node, reqs = make_requests(rng, n, GAS_LENGTHS)
    p = len(reqs)
    req = np.zeros((p, c, q), np.int64)
    mask = np.zeros((p, c), np.uint32)
    ncont = (np.arange(p) % c + 1).astype(np.int32)
    for pi in range(p):
        for ci in range(ncont[pi]):
            num = (0, 1, 3, 65 + int(rng.integers(0, 200)))[(pi + ci) % 4]
            mask[pi, ci] = int(rng.integers(0, 1 << (q - 1))) << 1 | (1 if num else 0)
            req[pi, ci, 0] = num
            req[pi, ci, 1:] = rng.integers(0, 400, q - 1) * max(num, 1)
    sel = [sum(int(req[pi, ci, 0]) for ci in range(ncont[pi])) for pi in range(p)]
    assert {0, 1} & set(sel) and any(s == 3 for s in req[:, :, 0].ravel()) and max(sel) > 64
    assert set(ncont) == {1, 2, 3, 4}
    mask[2, 0] |= UNKNOWN_KIND
    req[2, 0, 0], mask[2, 0] = 1, mask[2, 0] | 1  # with an i915 request: fits no node
    return n_cards, cap, used, off, node, reqs, req, mask, ncont


@pytest.mark.gpu
@pytest.mark.parametrize("k,n", [(8, 500), (12, 500), (64, 12)])
def test_gas_fit_requests_matches_oracle_gathered_to_positions(ctx, oracle, k, n):
    import torch
    rng = np.random.default_rng(900 + k)
    n_cards, cap, used, off, node, reqs, req, mask, ncont = gas_case(rng, n, k)
    assert -1 in n_cards and 0 in n_cards
    _gen[0] += 1
    gen = _gen[0]
    ctx.gas_snapshot_set(gen, n_cards, cap, used)
    fill = np.uint64(0x5A5A5A5A5A5A5A5A)
    ld = w64(300) + 2
    for i915 in (0, -1):
        words = oracle.gas_fit(n_cards, cap, used, req, mask, ncont, i915)
        want = [gather_bits((words[r] >> 31).astype(bool), rq, False)
                for r, rq in enumerate(reqs)]
        if i915 == 0:
            allw = np.concatenate(want)
            assert 0.02 < allw.mean() < 0.98
            assert not want[2].any()  # the unknown kind
        rows = ctx.gas_fit_requests(gen, off, node, req, mask, ncont, i915,
                                    out=np.full((len(reqs), ld), fill, np.uint64))
        check_rows(rows, reqs, want, fill, f"host i915 {i915}")
        fit_t = torch.from_numpy(np.full((len(reqs), ld), fill, np.uint64).view(np.int64)).cuda()
        ctx.gas_fit_requests_device(
            gen, off, torch.from_numpy(node).cuda(), req.shape[1], i915,
            torch.from_numpy(req).cuda(), torch.from_numpy(mask.view(np.int32)).cuda(),
            torch.from_numpy(ncont).cuda(), fit_t, ld, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        check_rows(fit_t.cpu().numpy().view(np.uint64), reqs, want, fill, f"device i915 {i915}")
    # nothing resident was written, the generation did not move
    g, after = ctx.gas_snapshot_get()
    assert g == gen
    np.testing.assert_array_equal(after, used)
    with pytest.raises(pas_amd.PasError) as e:
        ctx.gas_fit_requests(gen + 1, off, node, req, mask, ncont, 0)
    assert e.value.code == _lib.PAS_ESTALE
    bad = ncont.copy()
    bad[1] = req.shape[1] + 1
    with pytest.raises(pas_amd.PasError) as e:
        ctx.gas_fit_requests(gen, off, node, req, mask, bad, 0)
    assert e.value.code == _lib.PAS_EINVAL
