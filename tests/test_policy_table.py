"""The resident policy table and the verbs by policy id (pas_tas_policies_set,
pas_tas_policies_violated, pas_tas_eval_policies, pas_tas_filter_requests_policies and their
_device forms) against the oracle called per pod or per request with the policy's own rules.

The snapshot is test_request_batch.py's column mix: milli with few distinct values, scale 0,
scale 7 and one wide column, about 20 % of the nodes absent per column, at N = 3000 (not a
multiple of 64, an odd number of words per row), N = 64 and N = 1."""
import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from helpers import pack_bits, unpack_bits, w64
from oracle import RULE_DTYPE

M, WIDE = 4, 3
SCALE = [3, 0, 7, 3]
I32_MAX = 2**31 - 1
LT, GT, EQ = 0, 1, 2
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 300, 700]
NEW = ("pas_tas_policies_set", "pas_tas_policies_info", "pas_tas_policies_drop",
       "pas_tas_policies_violated", "pas_tas_policies_violated_device", "pas_tas_eval_policies",
       "pas_tas_eval_policies_device", "pas_tas_filter_requests_policies",
       "pas_tas_filter_requests_policies_device")


# ------------------------------------------------------------------------- snapshot, table

class Snap:
    pass


def make_snapshot(n, seed):
    """n x 4 columns as the request-batch tests': t.v / t.whole / t.nano are what the library
    takes, t.u / t.s the oracle's per-value decimal form of the same values."""
    rng = np.random.default_rng(seed)
    t = Snap()
    t.n = n
    k = rng.integers(0, 5, (M, n)).astype(np.int64)
    v = np.zeros((M, n), np.int64)
    v[0] = k[0] * 1000
    v[0, ::97] = rng.integers(-2**62, 2**62, len(range(0, n, 97)))
    v[1] = k[1]
    v[2] = k[2] * 10**7 + rng.integers(0, 2, n)
    whole = rng.choice(np.arange(-3, 4), n).astype(np.int64)
    nano = rng.choice(np.array([0, 0, 1, 500_000_000, 999_999_999], np.uint32), n)
    big = rng.random(n) < 0.2
    whole[big] = rng.choice(rng.integers(-2**62, 2**62, 6), int(big.sum()))
    nano[big] = 0
    t.pres_b = rng.random((M, n)) >= 0.2
    t.pres = pack_bits(t.pres_b)
    t.v, t.whole, t.nano = v, whole, nano
    t.u = v.copy()
    t.s = np.repeat(np.array(SCALE, np.int8)[:, None], n, axis=1)
    frac = nano != 0
    t.u[WIDE] = np.where(frac, whole * 10**9 + nano.astype(np.int64), whole)
    t.s[WIDE] = np.where(frac, 9, 0)
    return t


def install(c, t, gen):
    """The snapshot into context c, ending at generation gen."""
    c.tas_snapshot_set(gen - 1, t.v, t.pres, SCALE)
    c.tas_snapshot_update_wide(gen - 1, gen, [WIDE], t.whole[None], t.nano[None],
                               t.pres[WIDE:WIDE + 1])
    assert c.tas_snapshot_wide_count() == 1
    t.gen = gen


def rules_of(triples):
    r = np.zeros(len(triples), RULE_DTYPE)
    for i, x in enumerate(triples):
        r[i] = x
    return r


def make_table(seed=0x7AB1):
    """The 8 policies: [(dontschedule rules, prio rule)]."""
    rng = np.random.default_rng(seed)
    many = np.zeros(16, RULE_DTYPE)
    many["metric"] = rng.choice([0, 1, 2, WIDE], 16)
    many["op"] = rng.integers(0, 3, 16)
    many["target"] = rng.choice([0, 1, 2, 3, 4, 9, -9], 16)
    many[0] = (-1, GT, 0)      # a metric that is not cached
    many[1] = (M + 3, LT, 5)   # past the snapshot's columns: not cached either
    many[2] = (WIDE, EQ, 1)
    many[3] = (2, GT, 3)
    same = rules_of([(0, GT, 2), (2, LT, 1)])
    return [
        (rules_of([]), (0, GT, 0)),                                    # no dontschedule rules
        (rules_of([(-1, GT, 0)]), (1, LT, 0)),                         # only column -1
        (rules_of([(WIDE, LT, -1), (WIDE, GT, 2), (WIDE, EQ, 0)]), (WIDE, GT, 0)),
        (many, (2, LT, 0)),                                            # 16 rules
        (same, (0, LT, 0)),                                            # two identical policies
        (same.copy(), (0, LT, 0)),
        (rules_of([(1, LT, 2)]), (-1, 0, 0)),                          # no prio rule
        (rules_of([(1, EQ, 3)]), (1, EQ, 0)),                          # Equals at a tied value
    ]


def table_arrays(table):
    rules = np.concatenate([r for r, _ in table]) if table else np.zeros(0, RULE_DTYPE)
    off = np.concatenate([[0], np.cumsum([len(r) for r, _ in table])]).astype(np.int32)
    return rules, off, rules_of([p for _, p in table])


def per_pod(table, ids):
    """The per-pod CSR and prio the parent's pas_tas_eval takes for pods of these policy ids
    (an id outside the table: no rules, no prio rule)."""
    rs, off, prio = [], [0], []
    for i in ids:
        r, p = table[i] if 0 <= i < len(table) else (rules_of([]), (-1, 0, 0))
        rs.append(r)
        off.append(off[-1] + len(r))
        prio.append(p)
    rules = np.concatenate(rs) if rs else np.zeros(0, RULE_DTYPE)
    return rules, np.array(off, np.int32), rules_of(prio)


def want_eval(oracle, t, table, ids, cand, flags):
    rules, off, prio = per_pod(table, ids)
    return oracle.tas_eval(t.u, t.pres, rules, off, prio, cand=cand, flags=flags, v_scale=t.s)


def check_eval(got, want, flags, what=""):
    gp, go, gl = got
    wp, wo, wl = want
    if flags & 1:
        np.testing.assert_array_equal(gp, wp, err_msg=f"{what}: pass")
    if flags & 2:
        np.testing.assert_array_equal(gl, wl, err_msg=f"{what}: order_len")
        for p in range(len(wl)):
            np.testing.assert_array_equal(go[p, : wl[p]], wo[p, : wl[p]],
                                          err_msg=f"{what}: order of pod {p}")


def make_ids(rng, n_pods, n_policies):
    ids = rng.integers(0, n_policies, n_pods).astype(np.int32)
    ids[: n_policies] = np.arange(n_policies)  # every policy
    ids[rng.choice(np.arange(n_policies, n_pods), 9, replace=False)] = -1
    return ids


def make_cand(rng, n_pods, n):
    return pack_bits(rng.random((n_pods, n)) < 0.7)


@pytest.fixture(scope="module")
def own():
    """A context of this module's own: the policy table and its snapshot stay as installed."""
    c = pas_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big(own):
    t = make_snapshot(3000, 0xBA7C)
    install(own, t, 90_002)
    t.table = make_table()
    own.tas_policies_set(*table_arrays(t.table))
    rng = np.random.default_rng(0x1D5)
    t.ids = make_ids(rng, 130, len(t.table))
    t.cand = make_cand(rng, 130, t.n)
    return t


# ------------------------------------------------------------------------- no GPU

def test_lib_declares_the_new_functions():
    for name in NEW:
        assert name in _lib.SIGNATURES, name
    for fam in ("pas_tas_policies_violated", "pas_tas_eval_policies",
                "pas_tas_filter_requests_policies"):
        assert len(_lib.SIGNATURES[fam + "_device"][1]) == len(_lib.SIGNATURES[fam][1]) + 1


# ------------------------------------------------------------------------- eval

@pytest.mark.gpu
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("with_cand", [True, False])
def test_eval_matches_oracle_per_pod(own, oracle, big, flags, with_cand):
    t = big
    assert own.tas_policies_info() == (8, sum(len(r) for r, _ in t.table))
    assert (t.ids == -1).sum() >= 9 and set(t.ids.tolist()) == set(range(-1, 8))
    cand = t.cand if with_cand else None
    got = own.tas_eval_policies(t.gen, t.ids, cand, flags)
    want = want_eval(oracle, t, t.table, t.ids, cand, flags)
    check_eval(got, want, flags)
    if flags & 1:
        # the cases are in the batch: a pod without a policy passes its candidates, the policy
        # on column -1 violates nothing, the two identical policies agree, verdicts differ
        none = int(np.nonzero(t.ids == -1)[0][0])
        full = pack_bits(np.ones((1, t.n), bool))[0]
        np.testing.assert_array_equal(got[0][none], cand[none] if with_cand else full)
        if not with_cand:
            np.testing.assert_array_equal(got[0][1], full)
            np.testing.assert_array_equal(got[0][4], got[0][5])
            assert len({got[0][p].tobytes() for p in range(8)}) >= 5
    if flags & 2:
        assert got[2][6] == 0 and got[2][int(np.nonzero(t.ids == -1)[0][0])] == 0
        assert got[2][2] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("with_cand", [True, False])
def test_eval_device_form_equals_host_form(own, big, flags, with_cand):
    import torch
    t = big
    P, W = len(t.ids), w64(t.n)
    cand = t.cand if with_cand else None
    hp, ho, hl = own.tas_eval_policies(t.gen, t.ids, cand, flags)
    ids_t = torch.from_numpy(t.ids).cuda()
    cand_t = torch.from_numpy(t.cand.view(np.int64)).cuda() if with_cand else None
    pass_t = torch.full((P, W), 0x55, dtype=torch.int64, device="cuda")
    order_t = torch.full((P, t.n), -5, dtype=torch.int32, device="cuda")
    len_t = torch.full((P,), -5, dtype=torch.int32, device="cuda")
    own.tas_eval_policies_device(t.gen, P, ids_t, cand_t, flags, pass_t, order_t, len_t,
                                 stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    if flags & 1:
        np.testing.assert_array_equal(pass_t.cpu().numpy().view(np.uint64), hp)
    else:
        assert (pass_t == 0x55).all()  # PRIORITIZE alone writes no pass row
    if flags & 2:
        np.testing.assert_array_equal(len_t.cpu().numpy(), hl)
        od = order_t.cpu().numpy()
        for p in range(P):
            np.testing.assert_array_equal(od[p, : hl[p]], ho[p, : hl[p]], err_msg=f"pod {p}")


@pytest.mark.gpu
def test_eval_unaligned_rows_take_the_word_path(own, oracle, big):
    # pass rows that start 8 bytes off a 16-byte boundary: the kernel's scalar form
    import torch
    t = big
    P, W = len(t.ids), w64(t.n)
    buf = torch.zeros(P * W + 1, dtype=torch.int64, device="cuda")
    pass_t = buf[1:]
    assert pass_t.data_ptr() % 16 == 8
    own.tas_eval_policies_device(t.gen, P, torch.from_numpy(t.ids).cuda(), None, 1, pass_t, None,
                                 None, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    want = want_eval(oracle, t, t.table, t.ids, None, 1)
    np.testing.assert_array_equal(pass_t.cpu().numpy().view(np.uint64).reshape(P, W), want[0])


@pytest.mark.gpu
def test_policies_violated_matches_oracle(own, oracle, big):
    import torch
    t = big
    rules, off, _ = table_arrays(t.table)
    want = oracle.tas_violations(t.u, t.pres, rules, off, v_scale=t.s)
    got = own.tas_policies_violated(t.gen)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, own.tas_violations(t.gen, rules, off))
    assert got[0].sum() == 0 and got[1].sum() == 0 and got[2].any() and got[7].any()
    out_t = torch.full(got.shape, 0x55, dtype=torch.int64, device="cuda")
    own.tas_policies_violated_device(t.gen, out_t, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_t.cpu().numpy().view(np.uint64), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 1])
def test_eval_at_the_word_boundaries(oracle, n):
    t = make_snapshot(n, 0xB0 + n)
    t.pres_b[:, 0] = True  # (N = 1: the node has every metric)
    t.pres = pack_bits(t.pres_b)
    table = make_table()
    rng = np.random.default_rng(n)
    ids = make_ids(rng, 20, len(table))
    cand = make_cand(rng, 20, n)
    with pas_amd.Context(0) as c:
        install(c, t, 91_000 + 2 * n)
        c.tas_policies_set(*table_arrays(table))
        for flags in (1, 2, 3):
            for cd in (cand, None):
                got = c.tas_eval_policies(t.gen, ids, cd, flags)
                check_eval(got, want_eval(oracle, t, table, ids, cd, flags), flags,
                           f"N {n} flags {flags} cand {cd is not None}")
        rules, off, _ = table_arrays(table)
        np.testing.assert_array_equal(c.tas_policies_violated(t.gen),
                                      oracle.tas_violations(t.u, t.pres, rules, off,
                                                            v_scale=t.s))
        req = np.array([0, -1, n - 1, n, 0, I32_MAX], np.int32)
        pol = np.array([3, 7, -1], np.int32)
        rows = c.tas_filter_requests_policies(t.gen, [0, 2, 2, 6], pol, req)
        check_request_rows(oracle, t, table, rows, [req[:2], req[2:2], req[2:]], pol)


# ------------------------------------------------------------------------- request filter

def make_requests(rng, n_nodes, lengths):
    """test_request_batch.py's requests: mostly distinct nodes, about 10 % repeats, about 5 %
    ids the snapshot does not hold, one request of unknown ids only."""
    reqs = []
    for n in lengths:
        req = rng.permutation(n_nodes)[np.arange(n) % n_nodes].astype(np.int32)
        for j in np.nonzero(rng.random(n) < 0.1)[0]:
            if j:
                req[j] = req[rng.integers(0, j)]
        req[rng.random(n) < 0.05] = rng.choice([-1, n_nodes, I32_MAX, -7, n_nodes + 5])
        if n > 70:
            req[2] = abs(int(req[2])) % n_nodes
            req[70] = req[2]  # a repeat more than a wave apart
        if n > 5:
            req[1], req[3], req[5] = -1, n_nodes, I32_MAX
        reqs.append(req)
    reqs.append(rng.choice([-1, n_nodes, I32_MAX], 100).astype(np.int32))
    off = np.concatenate([[0], np.cumsum([len(r) for r in reqs])]).astype(np.int32)
    return off, np.concatenate(reqs).astype(np.int32), reqs


def want_request_bits(oracle, t, table, reqs, pol):
    """Per request: the oracle's filter with the request's policy's rules over every node,
    gathered to the request's positions; a node the snapshot does not hold passes."""
    rules, off, prio = per_pod(table, pol)
    prio["metric"] = -1
    ok, _, _ = oracle.tas_eval(t.u, t.pres, rules, off, prio, flags=1, v_scale=t.s)
    ok = unpack_bits(ok, t.n)
    out = []
    for r, req in enumerate(reqs):
        req = np.asarray(req, np.int64)
        known = (req >= 0) & (req < t.n)
        bits = np.ones(len(req), bool)
        bits[known] = ok[r][req[known]]
        out.append(bits)
    return out


def check_request_rows(oracle, t, table, rows, reqs, pol, fill=None):
    want = want_request_bits(oracle, t, table, reqs, pol)
    for r, req in enumerate(reqs):
        n, words = len(req), w64(len(req))
        got = unpack_bits(rows[r, :words], words * 64) if words else np.zeros(0, bool)
        np.testing.assert_array_equal(got[:n], want[r], err_msg=f"request {r} (n {n})")
        assert not got[n:].any(), f"request {r}: bits past the request's length"
        if fill is not None:
            assert (rows[r, words:] == fill).all(), f"request {r}: words past its own"


@pytest.fixture(scope="module")
def requests(big):
    rng = np.random.default_rng(0x4E0)
    off, req, reqs = make_requests(rng, big.n, LENGTHS)
    pol = (np.arange(len(reqs)) % 8).astype(np.int32)
    pol[[2, 6]] = -1
    # the longest requests meet the policies with the most rules
    pol[len(LENGTHS) - 1], pol[len(LENGTHS) - 2] = 3, 2
    return off, req, reqs, pol


@pytest.mark.gpu
def test_filter_requests_match_oracle_per_request(own, oracle, big, requests):
    off, req, reqs, pol = requests
    assert {len(r) for r in reqs} >= set(LENGTHS)
    rows = own.tas_filter_requests_policies(big.gen, off, pol, req)
    assert rows.shape == (len(reqs), w64(700))
    check_request_rows(oracle, big, big.table, rows, reqs, pol)
    # and the parent's verb with the same rules per request
    rules, rule_off, _ = per_pod(big.table, pol)
    np.testing.assert_array_equal(rows, own.tas_filter_requests(big.gen, off, rules, rule_off,
                                                                req))
    fill = np.uint64(0x5555555555555555)
    out = np.full((len(reqs), w64(700) + 3), fill, np.uint64)
    own.tas_filter_requests_policies(big.gen, off, pol, req, out=out)
    check_request_rows(oracle, big, big.table, out, reqs, pol, fill)


@pytest.mark.gpu
def test_filter_requests_device_form(own, oracle, big, requests):
    import torch
    off, req, reqs, pol = requests
    ld = w64(700) + 2
    fill = 0x5555555555555555
    req_t = torch.from_numpy(req).cuda()
    rows_t = torch.full((len(reqs), ld), fill, dtype=torch.int64, device="cuda")
    own.tas_filter_requests_policies_device(big.gen, off, pol, req_t, rows_t, ld,
                                            stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    rows = rows_t.cpu().numpy().view(np.uint64)
    check_request_rows(oracle, big, big.table, rows, reqs, pol, np.uint64(fill))
    # ids outside the table are read as -1
    bad = pol.copy()
    bad[[0, 4, 9]] = [-7, 8, I32_MAX]
    own.tas_filter_requests_policies_device(big.gen, off, bad, req_t, rows_t, ld,
                                            stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    as_none = bad.copy()
    as_none[[0, 4, 9]] = -1
    check_request_rows(oracle, big, big.table, rows_t.cpu().numpy().view(np.uint64), reqs,
                       as_none, np.uint64(fill))
    with pytest.raises(pas_amd.PasError) as e:
        own.tas_filter_requests_policies(big.gen, off, bad, req)
    assert e.value.code == _lib.PAS_EINVAL


# ------------------------------------------------------------------------- invalidation

@pytest.mark.gpu
def test_invalidation_in_order_on_one_context(oracle):
    t = make_snapshot(3000, 0x1A7)
    table = make_table()
    rng = np.random.default_rng(0x1A8)
    ids = make_ids(rng, 40, len(table))
    cand = make_cand(rng, 40, t.n)

    def check(c, what, cd=cand):
        for flags in (1, 3):
            check_eval(c.tas_eval_policies(t.gen, ids, cd, flags),
                       want_eval(oracle, t, table, ids, cd, flags), flags, what)
        return c.tas_eval_policies(t.gen, ids, None, 1)[0]

    with pas_amd.Context(0) as c:
        install(c, t, 92_002)
        c.tas_policies_set(*table_arrays(table))
        before = check(c, "1. first evaluation")
        # 2. a column refresh that changes verdicts: a stale bitmap fails here
        t.v[1] = 4 - t.v[1]
        t.u[1] = t.v[1]
        c.tas_snapshot_update(t.gen, t.gen + 1, [1], t.v[1:2], t.pres[1:2])
        t.gen += 1
        after = check(c, "2. after pas_tas_snapshot_update")
        assert not np.array_equal(before[6], after[6]) and not np.array_equal(before[7], after[7])
        # 3. a compaction that drops nodes
        src = np.nonzero(rng.random(t.n) >= 0.1)[0].astype(np.int32)
        c.tas_snapshot_compact(t.gen, t.gen + 1, src)
        t.gen += 1
        for name in ("v", "u", "s", "pres_b"):
            setattr(t, name, np.ascontiguousarray(getattr(t, name)[:, src]))
        t.whole, t.nano, t.n = t.whole[src], t.nano[src], len(src)
        t.pres = pack_bits(t.pres_b)
        cand = make_cand(rng, 40, t.n)
        check(c, "3. after pas_tas_snapshot_compact", cand)
        # 4. the table with one policy changed
        table[6] = (rules_of([(1, GT, 1), (2, EQ, 2)]), (2, GT, 0))
        before = c.tas_eval_policies(t.gen, ids, None, 1)[0]
        c.tas_policies_set(*table_arrays(table))
        after = check(c, "4. after pas_tas_policies_set", cand)
        assert not np.array_equal(before[6], after[6])
        # 5. a reshape that moves a column: the table's metric indices name other columns now
        move = [1, 0, 2, 3]
        c.tas_snapshot_reshape(t.gen, t.gen + 1, t.n, M, move)
        t.gen += 1
        with pytest.raises(pas_amd.PasError) as e:
            c.tas_eval_policies(t.gen, ids, cand, 1)
        assert e.value.code == _lib.PAS_ESTALE and "policy table" in str(e.value)
        with pytest.raises(pas_amd.PasError) as e:
            c.tas_policies_violated(t.gen)
        assert e.value.code == _lib.PAS_ESTALE and "policy table" in str(e.value)
        with pytest.raises(pas_amd.PasError) as e:
            c.tas_filter_requests_policies(t.gen, [0, 1], [0], [0])
        assert e.value.code == _lib.PAS_ESTALE and "policy table" in str(e.value)
        for name in ("v", "u", "s", "pres_b"):
            setattr(t, name, np.ascontiguousarray(getattr(t, name)[move]))
        t.pres = pack_bits(t.pres_b)
        new_col = {0: 1, 1: 0, 2: 2, 3: 3, -1: -1, M + 3: M + 3}

        def renamed(r):
            r = r.copy()
            r["metric"] = [new_col[int(m)] for m in r["metric"]]
            return r
        table = [(renamed(r), (new_col[p[0]], p[1], p[2])) for r, p in table]
        c.tas_policies_set(*table_arrays(table))
        check(c, "5. after pas_tas_snapshot_reshape and a new table", cand)
        # a wrong generation still names the generation
        with pytest.raises(pas_amd.PasError) as e:
            c.tas_eval_policies(t.gen + 1, ids, cand, 1)
        assert e.value.code == _lib.PAS_ESTALE and "generation" in str(e.value)
        # 6. no table
        c.tas_policies_drop()
        for call in (lambda: c.tas_eval_policies(t.gen, ids, cand, 1),
                     lambda: c.tas_policies_violated(t.gen),
                     lambda: c.tas_policies_info(),
                     lambda: c.tas_filter_requests_policies(t.gen, [0, 1], [0], [0])):
            with pytest.raises(pas_amd.PasError) as e:
                call()
            assert e.value.code == _lib.PAS_EINVAL
        c.tas_policies_set(*table_arrays(table))  # and a table again
        check(c, "6. after pas_tas_policies_drop and a new table", cand)


@pytest.mark.gpu
def test_table_needs_a_snapshot_and_takes_an_empty_table(oracle):
    with pas_amd.Context(0) as c:
        with pytest.raises(pas_amd.PasError) as e:
            c.tas_policies_set(*table_arrays(make_table()))
        assert e.value.code == _lib.PAS_ENOSNAP
        t = make_snapshot(200, 5)
        install(c, t, 93_002)
        c.tas_policies_set(*table_arrays([]))
        assert c.tas_policies_info() == (0, 0)
        assert c.tas_policies_violated(t.gen).shape == (0, w64(200))
        ids = np.full(3, -1, np.int32)
        check_eval(c.tas_eval_policies(t.gen, ids, None, 3),
                   want_eval(oracle, t, [], ids, None, 3), 3)
        # a snapshot set after the table: stale, as after a reshape
        c.tas_policies_set(*table_arrays(make_table()))
        install(c, t, 93_004)
        with pytest.raises(pas_amd.PasError) as e:
            c.tas_eval_policies(t.gen, ids, None, 1)
        assert e.value.code == _lib.PAS_ESTALE and "policy table" in str(e.value)


# ------------------------------------------------------------------------- two streams

@pytest.mark.gpu
def test_build_on_one_stream_read_on_another(oracle):
    import torch
    t = make_snapshot(3000, 0x25)
    table = make_table()
    rng = np.random.default_rng(0x26)
    ids = make_ids(rng, 130, len(table))
    P, W = len(ids), w64(t.n)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    ids_t = torch.from_numpy(ids).cuda()
    pa = torch.zeros((P, W), dtype=torch.int64, device="cuda")
    pb = torch.zeros((P, W), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pas_amd.Context(0) as c:
        install(c, t, 94_002)
        c.tas_policies_set(*table_arrays(table))
        c.tas_eval_policies_device(t.gen, P, ids_t, None, 1, pa, None, None, stream=a)  # builds
        c.tas_eval_policies_device(t.gen, P, ids_t, None, 1, pb, None, None, stream=b)
        torch.cuda.synchronize()
        want = want_eval(oracle, t, table, ids, None, 1)[0]
        np.testing.assert_array_equal(pa.cpu().numpy().view(np.uint64), want)
        np.testing.assert_array_equal(pb.cpu().numpy().view(np.uint64), want)


# ------------------------------------------------------------------------- malformed inputs

@pytest.mark.gpu
def test_ids_outside_the_table(own, oracle, big):
    import torch
    t = big
    ids = t.ids.copy()
    ids[[3, 50, 129]] = [-7, len(t.table), I32_MAX]
    for flags in (1, 3):
        with pytest.raises(pas_amd.PasError) as e:
            own.tas_eval_policies(t.gen, ids, t.cand, flags)
        assert e.value.code == _lib.PAS_EINVAL and "policy id" in str(e.value)
    P, W = len(ids), w64(t.n)
    pass_t = torch.zeros((P, W), dtype=torch.int64, device="cuda")
    order_t = torch.zeros((P, t.n), dtype=torch.int32, device="cuda")
    len_t = torch.zeros((P,), dtype=torch.int32, device="cuda")
    own.tas_eval_policies_device(t.gen, P, torch.from_numpy(ids).cuda(),
                                 torch.from_numpy(t.cand.view(np.int64)).cuda(), 3, pass_t,
                                 order_t, len_t, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    as_none = ids.copy()
    as_none[[3, 50, 129]] = -1
    got = (pass_t.cpu().numpy().view(np.uint64), order_t.cpu().numpy(), len_t.cpu().numpy())
    check_eval(got, want_eval(oracle, t, t.table, as_none, t.cand, 3), 3)


@pytest.mark.gpu
def test_unknown_operator_in_a_referenced_policy(oracle):
    t = make_snapshot(100, 0x77)
    t.pres_b[2] = False  # column 2 is cached with no node
    t.pres = pack_bits(t.pres_b)
    table = make_table()[:3]
    table.append((rules_of([(1, 3, 0)]), (-1, 0, 0)))  # unknown operator, non-empty column
    table.append((rules_of([(2, 3, 0)]), (-1, 0, 0)))  # the same rule on the empty column
    with pas_amd.Context(0) as c:
        install(c, t, 95_002)
        c.tas_policies_set(*table_arrays(table))  # accepted: nothing is evaluated yet
        for ids in ([0, 3, 1], [3]):
            with pytest.raises(pas_amd.PasError) as e:
                c.tas_eval_policies(t.gen, np.array(ids, np.int32), None, 1)
            assert e.value.code == _lib.PAS_EINVAL and "unknown operator" in str(e.value)
        with pytest.raises(pas_amd.PasError) as e:
            c.tas_filter_requests_policies(t.gen, [0, 0, 2], [3, 0], [0, 1])
        assert e.value.code == _lib.PAS_EINVAL and "unknown operator" in str(e.value)
        # the policy unreferenced, and the rule on the empty column: nobody evaluates them
        ids = np.array([0, 1, 2, 4, -1], np.int32)
        check_eval(c.tas_eval_policies(t.gen, ids, None, 3),
                   want_eval(oracle, t, table, ids, None, 3), 3)
        rows = c.tas_filter_requests_policies(t.gen, [0, 2, 4], [4, 2],
                                              np.array([0, 1, 5, 7], np.int32))
        check_request_rows(oracle, t, table, rows,
                           [np.array([0, 1], np.int32), np.array([5, 7], np.int32)], [4, 2])
