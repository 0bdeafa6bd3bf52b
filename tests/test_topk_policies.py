"""The top-k entry points by policy id (pas_tas_topk_policies[_wide]_device,
pas_tas_gas_topk_policies[_wide][_after]_device) and what is built on them
(place_to_completion(pod_policy_t=), ShardedTopK.run_policies / run_tas_gas_policies,
PolicyCache.ids_of).

Contract (include/pas.h): each entry point gives exactly the outputs of its counterpart without
_policies called with pod p's rules and prio being table row d_pod_policy[p].  So the expected
value is the counterpart itself, called with the per-pod CSR and prio built from the table
(per_pod of test_policy_table.py); the counterparts are pinned to the oracle by
test_shard.py, test_topk_wide.py and test_topk_after.py.  One small case is checked against the
oracle directly.  All outputs are compared for equality, the padding records included; the
output buffers are filled with another value first, so an unwritten record fails too.

The snapshot and table are test_policy_table.py's (four columns at scales 3 / 0 / 7 and one
wide, about 20 % absent, 8 policies) with three more policies: one of 40 rules whose last rule
is on its own prioritize metric (the jump loop's second batch of 32 rules), and two whose
rules exclude the head and the middle of their own order, prioritizing GreaterThan and
LessThan (column 0 has five distinct values, so the excluded ranges are hundreds of positions
long)."""
import ctypes

import numpy as np
import pytest

import pas_amd
from pas_amd import _lib
from pas_amd.policy_cache import PolicyCache, TasPolicy
from helpers import w64
from test_policy_table import (EQ, GT, LT, M, SCALE, WIDE, install, make_snapshot, make_table,
                               per_pod, rules_of, table_arrays)

I64_MIN, I64_MAX = -2**63, 2**63 - 1
I32_MIN, I32_MAX, U32_MAX = -2**31, 2**31 - 1, 2**32 - 1
NEW = ("pas_tas_topk_policies_device", "pas_tas_topk_policies_wide_device",
       "pas_tas_gas_topk_policies_device", "pas_tas_gas_topk_policies_wide_device",
       "pas_tas_gas_topk_policies_after_device", "pas_tas_gas_topk_policies_wide_after_device")
BASE = 1234
P_MAX, C = 96, 4
FILL = -3  # what the output buffers hold before a call


# ------------------------------------------------------------------------- no GPU

def test_symbols_and_signatures():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        # the counterpart's arguments with (n_rules, rules, rule_off, prio) replaced by one
        # pointer: the policy ids
        rt, args = _lib.SIGNATURES[name.replace("_policies", "")]
        at = 3 if name.startswith("pas_tas_topk") else 4  # ctx, gen[s], n_pods
        assert args[at:at + 4] == [ctypes.c_int32] + [ctypes.c_void_p] * 3
        assert _lib.SIGNATURES[name] == (rt, args[:at] + [ctypes.c_void_p] + args[at + 4:])
    assert pas_amd.LIB.pas_abi_version() == 3


def test_context_has_the_methods():
    for name in NEW:
        assert callable(getattr(pas_amd.Context, name[len("pas_"):]))


def test_null_context():
    for name in NEW:
        args = [0 if a is not ctypes.c_void_p else None for a in _lib.SIGNATURES[name][1]]
        assert getattr(pas_amd.LIB, name)(*args) == _lib.PAS_EINVAL, name


class _TableCtx:
    """The part of a context PolicyCache calls (the fake of test_policy_cache.py)."""

    def __init__(self):
        self.tables = []

    def tas_policies_set(self, rules, rule_off, prio):
        self.tables.append((rules, rule_off, prio))


def test_policy_cache_ids_of():
    cache = PolicyCache(_TableCtx(), metric_names=["a", "b"])
    pols = [TasPolicy("ns", f"p{i}", {"dontschedule": [("a", "GreaterThan", i)]})
            for i in range(4)]
    for pol in pols:
        cache.on_add(pol)
    keys = [("ns", "p2"), ("ns", "absent"), ("ns", "p0"), ("other", "p1"), ("ns", "p3"),
            ("ns", "p2")]
    ids = cache.ids_of(keys)
    assert ids.dtype == np.int32 and ids.shape == (6,)
    assert ids.tolist() == [2, -1, 0, -1, 3, 2]
    assert [cache.id_of(k) for k in keys if k in cache.ids] == [2, 0, 3, 2]
    # a deleted policy is not held any more; its id goes to the next new policy
    cache.on_delete(pols[0])
    assert cache.ids_of([("ns", "p0"), ("ns", "p1")]).tolist() == [-1, 1]
    cache.on_add(TasPolicy("ns", "new", {}))
    assert cache.ids_of([("ns", "new"), ("ns", "p0")]).tolist() == [0, -1]
    assert cache.ids_of([]).shape == (0,) and cache.ids_of([]).dtype == np.int32


# ------------------------------------------------------------------------- the case

def full_table():
    """test_policy_table's 8 policies and: 8 = 40 rules, the last on its own prioritize metric;
    9 / 10 = rules on the prioritize metric that exclude the head and the middle of the order,
    prioritizing GreaterThan / LessThan."""
    rng = np.random.default_rng(0x70B)
    long_rules = [(int(rng.integers(0, M)), LT, -10**6) for _ in range(39)] + [(0, EQ, 3)]
    return make_table() + [
        (rules_of(long_rules), (0, LT, 0)),
        (rules_of([(0, GT, 3), (0, EQ, 1)]), (0, GT, 0)),
        (rules_of([(0, LT, 1), (0, EQ, 2)]), (0, LT, 0)),
    ]


N_POLICIES = 11


def make_ids(p):
    """p = 96: every row, -1, n_policies, INT32_MIN, INT32_MAX and random rows; 9: the three
    new policies, the wide one, the 16-rule one and the four ids outside the table; 1: the
    jumping policy alone."""
    outside = [-1, N_POLICIES, I32_MIN, I32_MAX]
    if p == 1:
        return np.array([9], np.int32)
    if p == 9:
        return np.array([8, 9, 10, 2, 3] + outside, np.int32)
    rng = np.random.default_rng(0x1D + p)
    ids = rng.integers(0, N_POLICIES, p).astype(np.int32)
    ids[:N_POLICIES] = np.arange(N_POLICIES)
    ids[N_POLICIES:N_POLICIES + 4] = outside
    ids[20:24] = [-7, N_POLICIES + 1, 2**30, -1]
    return ids


def pack(bits):
    """[P][n] bool -> [P][W64] uint64."""
    p, n = bits.shape
    padded = np.zeros((p, w64(n) * 64), bool)
    padded[:, :n] = bits
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64)


def narrowed(t):
    """The snapshot with column 3 narrow (milli): what the 64-bit record forms take."""
    t.v = t.v.copy()
    t.v[WIDE] = np.clip(t.whole, -5, 5) * 1000 + (t.nano // 1_000_000).astype(np.int64)
    t.u, t.s = t.v.copy(), np.repeat(np.array(SCALE, np.int8)[:, None], t.n, axis=1)
    return t


def tight_gas(rng, n, cards, p):
    """random_gas as test_topk_after.py uses it (3 kinds, 4 containers, capacities x 4); pods
    7 and 8 ask one GPU for more than a card holds: they fit nowhere."""
    from test_gas_gpu import random_gas
    nc, cap, used, req, mask, ncont = random_gas(rng, n, cards, 3, p, C, i915=0)
    cap *= 4
    req[7:9, 0, :2], mask[7:9, 0], ncont[7:9] = (1, 10**9), 0b111, 1
    return (nc, cap, used), (req, mask, ncont)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Case:
    """A snapshot pair and the table on a context, and the pod batch on the device."""
    _gen = [610_000]

    def __init__(self, c, n, wide, cards=8, seed=0x70C, table=None):
        Case._gen[0] += 10
        g = Case._gen[0]
        self.c, self.n, self.wide = c, n, wide
        self.t = t = make_snapshot(n, seed + n)
        if wide:
            install(c, t, g)
        else:
            narrowed(t)
            c.tas_snapshot_set(g, t.v, t.pres, SCALE)
            t.gen = g
        self.table = full_table() if table is None else table
        c.tas_policies_set(*table_arrays(self.table))
        rng = np.random.default_rng(seed ^ n)
        self.gs, self.gb = tight_gas(rng, n, cards, P_MAX)
        self.gas_gen = g + 5
        c.gas_snapshot_set(self.gas_gen, *self.gs)
        self.cand = pack(rng.random((P_MAX, n)) < 0.5)
        req, mask, ncont = self.gb
        self.gas_t = (dev(req), dev(mask.view(np.int32)), dev(ncont))

    def outputs(self, p, k):
        import torch
        key = torch.full((p, k), FILL, dtype=torch.int64, device="cuda")
        sub = torch.full((p, k), FILL, dtype=torch.int32, device="cuda")
        node = torch.full((p, k), FILL, dtype=torch.int32, device="cuda")
        ln = torch.full((p,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # the fills, before a call on another stream writes
        return (key, sub, node, ln) if self.wide else (key, node, ln)

    def topk(self, ids, k, gas=True, cand=False, after=None, policies=True, base=BASE,
             stream=None, sync=True):
        """Records as numpy (key, [sub,] node, len) of the first len(ids) pods; policies =
        False: the counterpart without _policies on the per-pod rules of the same ids."""
        p = len(ids)
        c, w = self.c, "_wide" if self.wide else ""
        cand_t = dev(self.cand[:p].view(np.int64)) if cand else None
        if policies:
            lead, name = (p, dev(np.asarray(ids, np.int32)), cand_t), "_policies"
        else:
            rules, off, prio = per_pod(self.table, ids)
            lead = (p, len(rules), dev(rules.view(np.uint8)), dev(off), dev(prio.view(np.uint8)),
                    cand_t)
            name = ""
        outs = self.outputs(p, k)
        if gas:
            cur = ()
            if after is not None:
                cur = [dev(after[0].astype(np.int64))]
                if self.wide:
                    cur.append(dev(after[1].astype(np.uint32).view(np.int32)))
                cur.append(dev(after[-1].astype(np.int32)))
                w += "_after"
            fn = getattr(c, f"tas_gas_topk{name}{w}_device")
            fn(self.t.gen, self.gas_gen, *lead, C, 0, *self.gas_t, k, base, *cur, *outs,
               stream=stream)
        else:
            fn = getattr(c, f"tas_topk{name}{w}_device")
            fn(self.t.gen, *lead, k, base, *outs, stream=stream)
        if not sync:
            return outs
        c.synchronize()
        return self.numpy(outs)

    def numpy(self, outs):
        got = [a.cpu().numpy() for a in outs]
        if self.wide:
            got[1] = got[1].view(np.uint32)
        return tuple(got)


def assert_same(got, want, what):
    names = ("key", "sub", "node", "len") if len(got) == 4 else ("key", "node", "len")
    for name, g, w in zip(names, got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")
    assert not (got[-1] == FILL).any(), what


@pytest.fixture(scope="module")
def own():
    c = pas_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big_narrow(own):
    return Case(own, 3000, False)


# ------------------------------------------------------------------------- shapes and ids

@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65, 3000])
def test_policy_forms_equal_their_counterparts(n, wide):
    with pas_amd.Context(0) as c:
        case = Case(c, n, wide)
        seen = 0
        for p in (1, 9, P_MAX):
            ids = make_ids(p)
            for k in (1, 16, 33, n + 5):
                for gas in (True, False):
                    for cand in (False, True):
                        what = f"N={n} P={p} k={k} gas={gas} cand={cand} wide={wide}"
                        got = case.topk(ids, k, gas=gas, cand=cand)
                        want = case.topk(ids, k, gas=gas, cand=cand, policies=False)
                        assert_same(got, want, what)
                        seen += int(got[-1].sum())
                        if k == n + 5:  # no list reaches k: padding in every row
                            assert (got[-1] < k).all() and (got[-2][:, -5:] == I32_MAX).all()
                        if p == P_MAX:  # ids outside the table: the empty list, padding only
                            out = (ids < 0) | (ids >= N_POLICIES)
                            assert out.sum() >= 7 and (got[-1][out] == 0).all()
                            assert (got[0][out] == I64_MAX).all()
                        if p == P_MAX and gas and n == 3000 and not cand:
                            assert got[-1][7] == 0 and got[-1][8] == 0  # fit nowhere
        assert seen > 0 or n == 1  # (one node may lack every column)


@pytest.mark.gpu
def test_the_case_holds_what_it_claims(big_narrow):
    """The lists are long enough to need several rounds, the jumping policies have lists that
    begin behind an excluded range, and the table's policies give different lists."""
    case = big_narrow
    ids = make_ids(P_MAX)
    key, node, ln = case.topk(ids, 33, gas=False)
    assert (ln[:N_POLICIES] > 0).sum() >= 8 and ln[6] == 0  # (6: no prio rule)
    assert (ln == 33).sum() >= P_MAX // 2
    v0 = case.t.v[0]
    # policy 9 (GreaterThan order, rules GreaterThan 3 and Equals 1 on the same column): the
    # head of the order (the values above 3 000) is excluded, hundreds of nodes
    assert ((v0 > 3000) & case.t.pres_b[0]).sum() > 200
    assert ln[9] > 0 and (v0[node[9, :ln[9]] - BASE] <= 3000).all()
    assert (v0[node[9, :ln[9]] - BASE] != 1000).all()
    assert ln[10] > 0 and (v0[node[10, :ln[10]] - BASE] >= 1000).all()
    # policy 8: the 40th rule (Equals 3 on its own column) is applied
    assert ln[8] > 0 and (v0[node[8, :ln[8]] - BASE] != 3000).all()
    assert len({node[p].tobytes() for p in range(N_POLICIES)}) >= 7


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
def test_seventeen_cards_take_the_scratch_shape(wide):
    with pas_amd.Context(0) as c:
        case = Case(c, 3000, wide, cards=17)
        assert c.gas_shape[1] == 17
        ids = make_ids(P_MAX)
        for cand in (False, True):
            got = case.topk(ids, 16, cand=cand)
            assert_same(got, case.topk(ids, 16, cand=cand, policies=False), f"cand={cand}")
            assert got[-1].sum() > 0


# ------------------------------------------------------------------------- the oracle itself

def canonical(v, scale):
    """(W, F) of pas.h for a narrow value v held at 10^scale."""
    w = v // 10**scale
    return w, (v - w * 10**scale) * 10**(9 - scale)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
def test_small_case_against_the_oracle(oracle, wide):
    n, k = 300, 4
    ids = make_ids(9)
    with pas_amd.Context(0) as c:
        case = Case(c, n, wide)
        t = case.t
        (nc, cap, used), (req, mask, ncont) = case.gs, case.gb
        fit = (oracle.gas_fit(nc, cap, used, req[:9], mask[:9], ncont[:9], 0) >> 31).astype(bool)
        rules, off, prio = per_pod(case.table, ids)
        for gas in (True, False):
            cand = pack(fit) if gas else None
            _, order, lens = oracle.tas_eval(t.u, t.pres, rules, off, prio, cand=cand, flags=3,
                                             v_scale=t.s)
            got = case.topk(ids, k, gas=gas, base=BASE)
            for p in range(9):
                lst = order[p, :lens[p]][:k].astype(np.int64)
                m, op = int(prio[p]["metric"]), int(prio[p]["op"])
                assert got[-1][p] == len(lst), (gas, p)
                assert got[-2][p, :len(lst)].tolist() == (lst + BASE).tolist(), (gas, p)
                assert (got[-2][p, len(lst):] == I32_MAX).all()
                assert (got[0][p, len(lst):] == I64_MAX).all()
                if not len(lst):
                    continue
                if wide:
                    if m == WIDE:
                        W, F = t.whole[lst], t.nano[lst].astype(np.int64)
                    else:
                        W, F = canonical(t.v[m, lst], SCALE[m])
                    wk = ~W if op == GT else W if op == LT else np.zeros_like(W)
                    ws = U32_MAX - F if op == GT else F if op == LT else np.zeros_like(F)
                    assert got[0][p, :len(lst)].tolist() == wk.tolist(), (gas, p)
                    assert got[1][p, :len(lst)].tolist() == ws.tolist(), (gas, p)
                    assert (got[1][p, len(lst):] == U32_MAX).all()
                else:
                    val = t.v[m, lst]
                    wk = ~val if op == GT else val if op == LT else np.zeros_like(val)
                    assert got[0][p, :len(lst)].tolist() == wk.tolist(), (gas, p)
            assert got[-1].sum() > 0


# ------------------------------------------------------------------------- forms

@pytest.mark.gpu
def test_record_forms_on_a_snapshot_with_a_wide_column():
    with pas_amd.Context(0) as c:
        case = Case(c, 300, True)
        ids = make_ids(9)
        case.wide = False  # the 64-bit forms on the same snapshot
        for gas in (True, False):
            with pytest.raises(pas_amd.PasError) as e:
                case.topk(ids, 4, gas=gas)
            assert e.value.code == _lib.PAS_ENOTEXACT
        cur = (np.full(9, I64_MIN), np.full(9, -1))
        with pytest.raises(pas_amd.PasError) as e:
            case.topk(ids, 4, after=cur)
        assert e.value.code == _lib.PAS_ENOTEXACT
        case.wide = True
        assert case.topk(ids, 4)[-1].sum() > 0


@pytest.mark.gpu
def test_argument_checks(big_narrow):
    import torch
    case, c = big_narrow, big_narrow.c
    ids_t = dev(make_ids(9))
    key, node, ln = case.outputs(9, 4)
    gas = (C, 0, *case.gas_t)

    def tas(gen=case.t.gen, p=9, ids=ids_t, k=4, base=0, outs=(key, node, ln)):
        c.tas_topk_policies_device(gen, p, ids, None, k, base, *outs)

    def both(tg=case.t.gen, gg=case.gas_gen, p=9, ids=ids_t, k=4, base=0, outs=(key, node, ln),
             g=gas):
        c.tas_gas_topk_policies_device(tg, gg, p, ids, None, *g, k, base, *outs)

    bad = [lambda: tas(ids=None), lambda: both(ids=None), lambda: tas(k=0), lambda: both(k=0),
           lambda: tas(base=-1), lambda: both(base=I32_MAX - 10), lambda: tas(p=-1),
           lambda: tas(outs=(None, node, ln)), lambda: both(outs=(key, None, ln)),
           lambda: both(outs=(key, node, None)), lambda: both(g=(C, 3, *case.gas_t)),
           lambda: both(g=(C, 0, None, case.gas_t[1], case.gas_t[2])),
           lambda: c.tas_gas_topk_policies_after_device(
               case.t.gen, case.gas_gen, 9, ids_t, None, *gas, 4, 0, None, None, key, node, ln)]
    for i, call in enumerate(bad):
        with pytest.raises(pas_amd.PasError) as e:
            call()
        assert e.value.code == _lib.PAS_EINVAL, i
    for call in (lambda: tas(gen=case.t.gen + 1), lambda: both(tg=case.t.gen + 1),
                 lambda: both(gg=case.gas_gen + 1)):
        with pytest.raises(pas_amd.PasError) as e:
            call()
        assert e.value.code == _lib.PAS_ESTALE and "generation" in str(e.value)
    # no pods: PAS_OK, nothing read or written, null arrays included
    tas(p=0, ids=None)
    both(p=0, ids=None)
    c.tas_gas_topk_policies_after_device(case.t.gen, case.gas_gen, 0, None, None, *gas, 4, 0,
                                         None, None, key, node, ln)
    c.synchronize()
    assert (key == FILL).all() and (node == FILL).all() and (ln == FILL).all()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------- resumption

def begin_cursor(case, p):
    return (np.full(p, I64_MIN),) + ((np.zeros(p, np.uint32),) if case.wide else ()) + \
        (np.full(p, -1),)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
def test_resumed_forms_equal_their_counterparts(wide):
    with pas_amd.Context(0) as c:
        case = Case(c, 3000, wide)
        ids = make_ids(P_MAX)
        p, k = P_MAX, 16
        first = case.topk(ids, k)
        whole = case.topk(ids, 3000)
        rng = np.random.default_rng(0xAF)
        mid = whole[-1] // 2  # inside the tie runs of columns 0 and 1 for most pods
        at = np.arange(p)
        end = (np.full(p, I64_MAX),) + ((np.full(p, U32_MAX),) if wide else ()) + \
            (np.full(p, I32_MAX),)
        cursors = {
            "begin": begin_cursor(case, p),
            "end": end,
            "each pod's k-th record": tuple(a[:, k - 1] for a in first[:-1]),
            "a record inside the list": tuple(a[at, mid] for a in whole[:-1]),
            "random bits": (rng.integers(I64_MIN, I64_MAX, p, endpoint=True),) +
            ((rng.integers(0, U32_MAX, p, endpoint=True),) if wide else ()) +
            (rng.integers(I32_MIN, I32_MAX, p, endpoint=True),),
            "small random": (rng.integers(-5, 5, p) * 1000,) +
            ((rng.choice([0, 1, 500_000_000, U32_MAX], p),) if wide else ()) +
            (rng.integers(BASE - 10, BASE + 3010, p),),
        }
        # (the tie runs are long: the middle record of most lists shares its key with others)
        tied = sum(int((whole[0][q, :whole[-1][q]] == whole[0][q, mid[q]]).sum() > 50)
                   for q in range(p) if whole[-1][q] > 0)
        assert tied >= p // 4
        for what, cur in cursors.items():
            for cand in (False, True):
                got = case.topk(ids, k, after=cur, cand=cand)
                want = case.topk(ids, k, after=cur, cand=cand, policies=False)
                assert_same(got, want, f"{what}, cand={cand}")
        assert_same(case.topk(ids, k, after=cursors["begin"]), first, "begin = the call itself")
        got = case.topk(ids, k, after=end)
        assert (got[-1] == 0).all() and (got[0] == I64_MAX).all() and (got[-2] == I32_MAX).all()
        got = case.topk(ids, k, after=cursors["each pod's k-th record"])
        np.testing.assert_array_equal(got[-2], whole[-2][:, k:2 * k])


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
def test_pages_of_seven_are_the_whole_list(wide):
    n, k = 300, 7
    with pas_amd.Context(0) as c:
        case = Case(c, n, wide)
        ids = make_ids(9)
        whole = case.topk(ids, n)
        assert whole[-1].max() > 5 * k
        cur = begin_cursor(case, 9)
        pages = []
        for _ in range(n // k + 2):
            page = case.topk(ids, k, after=cur)
            pages.append(page)
            cur = tuple(a[:, k - 1] for a in page[:-1])
            if (page[-1] == 0).all():
                break
        else:
            pytest.fail("the lists were not exhausted")
        for q in range(9):
            L = whole[-1][q]
            for j in range(len(whole) - 1):
                cat = np.concatenate([pg[j][q, :pg[-1][q]] for pg in pages])
                np.testing.assert_array_equal(cat, whole[j][q, :L], err_msg=f"pod {q}")


# ------------------------------------------------------------------------- state

@pytest.mark.gpu
def test_table_states_and_rebuilds():
    with pas_amd.Context(0) as c:
        case = Case(c, 3000, False)
        t, ids = case.t, make_ids(P_MAX)

        def check(what):
            """The TAS-only records (pods 7 and 8 fit no node)."""
            assert_same(case.topk(ids, 16), case.topk(ids, 16, policies=False), what)
            got = case.topk(ids, 16, gas=False)
            assert_same(got, case.topk(ids, 16, gas=False, policies=False), what + ", TAS only")
            return got
        before = check("1. first call")
        # 2. values move across a rule's target (policy 7: Equals 3 on column 1; 6: LessThan 2)
        t.v[1] = 4 - t.v[1]
        c.tas_snapshot_update(t.gen, t.gen + 1, [1], t.v[1:2], t.pres[1:2])
        t.gen += 1
        after = check("2. after pas_tas_snapshot_update")
        assert not np.array_equal(before[1][7], after[1][7])
        # 3. the table with one policy's rule changed
        before = after
        case.table[10] = (rules_of([(0, LT, 3)]), (0, LT, 0))
        c.tas_policies_set(*table_arrays(case.table))
        after = check("3. after pas_tas_policies_set")
        assert not np.array_equal(before[1][10], after[1][10])
        # 4. a reshape that moves a column: stale until the table is set again
        c.tas_snapshot_reshape(t.gen, t.gen + 1, t.n, M, [1, 0, 2, 3])
        t.gen += 1
        for gas in (True, False):
            with pytest.raises(pas_amd.PasError) as e:
                case.topk(ids, 16, gas=gas)
            assert e.value.code == _lib.PAS_ESTALE and "policy table" in str(e.value)
        with pytest.raises(pas_amd.PasError) as e:
            case.topk(ids, 16, after=begin_cursor(case, P_MAX))
        assert e.value.code == _lib.PAS_ESTALE and "policy table" in str(e.value)
        c.tas_policies_set(*table_arrays(case.table))
        check("4. after pas_tas_snapshot_reshape and pas_tas_policies_set")
        # 5. an empty table: every id reads as -1
        c.tas_policies_set(*table_arrays([]))
        for gas in (True, False):
            got = case.topk(ids, 16, gas=gas)
            assert (got[-1] == 0).all() and (got[0] == I64_MAX).all()
            assert (got[1] == I32_MAX).all()
        got = case.topk(ids, 16, after=begin_cursor(case, P_MAX))
        assert (got[-1] == 0).all() and (got[1] == I32_MAX).all()
        # 6. no table
        c.tas_policies_drop()
        for gas in (True, False):
            with pytest.raises(pas_amd.PasError) as e:
                case.topk(ids, 16, gas=gas)
            assert e.value.code == _lib.PAS_EINVAL


@pytest.mark.gpu
def test_build_on_one_stream_read_on_another():
    import torch
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with pas_amd.Context(0) as c:
        case = Case(c, 3000, False)
        ids = make_ids(P_MAX)
        want = case.topk(ids, 16, policies=False)
        torch.cuda.synchronize()
        ids_t = dev(ids)
        oa, ob = case.outputs(P_MAX, 16), case.outputs(P_MAX, 16)
        # a fresh table: the first call builds the violating sets on stream a; nothing
        # synchronizes the host between the two calls
        c.tas_policies_set(*table_arrays(case.table))
        torch.cuda.synchronize()
        for outs, s in ((oa, a), (ob, b)):
            c.tas_gas_topk_policies_device(case.t.gen, case.gas_gen, P_MAX, ids_t, None, C, 0,
                                           *case.gas_t, 16, BASE, *outs, stream=s)
        torch.cuda.synchronize()
        assert_same(case.numpy(oa), want, "stream a (builds)")
        assert_same(case.numpy(ob), want, "stream b (waits for the build's event)")


# ------------------------------------------------------------------------- the Python layer

def placement_inputs(wide):
    n, p = 200, 64
    rng = np.random.default_rng(0x91ACE + wide)
    t = make_snapshot(n, 0x91A)
    if not wide:
        narrowed(t)
    (nc, cap, used), (req, mask, ncont) = tight_gas(rng, n, 8, p)
    # little room: three nodes in five keep space on their first card for about one request,
    # the others for none, and most pods walk one of four orders: the pods take each other's
    # candidates and go through several rounds
    roomy = (rng.random(n) < 0.6)[:, None, None] & (np.arange(8) == 0)[None, :, None]
    used = np.maximum(used, cap[:, None, :] - np.where(roomy, 700, 1))
    used[np.arange(8)[None, :] >= nc[:, None]] = 0
    # pods 24 and up: one container asking one GPU for 500 of the second kind, so a roomy node
    # takes exactly one of them
    req[24:], mask[24:], ncont[24:] = 0, 0, 1
    req[24:, 0, :2], mask[24:, 0] = (1, 500), 0b011
    ids = make_ids(P_MAX)[:p].copy()
    ids[40:] = np.array([9, 10, 4, 0])[np.arange(p - 40) % 4]  # many pods on the same orders
    return t, (nc, cap, used), (req, mask, ncont), ids


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
def test_place_to_completion_by_policy_id(wide):
    import torch
    from pas_amd.placement import place_to_completion
    t, gs, (req, mask, ncont), ids = placement_inputs(wide)
    table = full_table()
    p, k = len(ids), 4
    results = []
    for by_id in (False, True):
        with pas_amd.Context(0) as c:
            if wide:
                install(c, t, 620_002)
            else:
                c.tas_snapshot_set(620_002, t.v, t.pres, SCALE)
            c.gas_snapshot_set(620_100, *gs)
            c.tas_policies_set(*table_arrays(table))
            gas_t = (dev(req), dev(mask.view(np.int32)), dev(ncont))
            if by_id:
                r = place_to_completion(c, 620_002, 620_100, p, 0, None, None, None, None, C, 0,
                                        *gas_t, k, node_base=BASE, wide=wide,
                                        pod_policy_t=dev(ids))
            else:
                rules, off, prio = per_pod(table, ids)
                r = place_to_completion(c, 620_002, 620_100, p, len(rules),
                                        dev(rules.view(np.uint8)), dev(off),
                                        dev(prio.view(np.uint8)), None, C, 0, *gas_t, k,
                                        node_base=BASE, wide=wide)
            torch.cuda.synchronize()
            results.append((r.node.cpu().numpy(), r.round.cpu().numpy(), r.res.cpu().numpy(),
                            r.n_placed, r.rounds, r.gas_gen, c.gas_snapshot_get()[1]))
    want, got = results
    for name, w, g in zip(("node", "round", "res", "n_placed", "rounds", "gas_gen", "used"),
                          want, got):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert got[3] > 0 and got[4] >= 2, (got[3], got[4])


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
def test_sharded_topk_by_policy_id(wide):
    import torch
    from pas_amd.shard import ShardedTopK
    with pas_amd.Context(0) as c:
        case = Case(c, 3000, wide)
        ids = make_ids(P_MAX)
        p, k = P_MAX, 16
        rules, off, prio = per_pod(case.table, ids)
        rule_t = (len(rules), dev(rules.view(np.uint8)), dev(off), dev(prio.view(np.uint8)))
        ids_t = dev(ids)
        cand_t = dev(case.cand.view(np.int64))
        topk = ShardedTopK(c, k, 1, 0, BASE, wide=wide)

        def lists(result):
            torch.cuda.synchronize()
            return result[0].cpu().numpy().copy(), result[1].cpu().numpy().copy()
        for cd in (None, cand_t):
            want = lists(topk.run(case.t.gen, p, *rule_t, cand_t=cd))
            got = lists(topk.run_policies(case.t.gen, p, ids_t, cand_t=cd))
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_array_equal(got[0], want[0])
            assert got[1].sum() > 0
            want = lists(topk.run_tas_gas(case.t.gen, case.gas_gen, p, *rule_t, C, 0,
                                          *case.gas_t, cand_t=cd))
            got = lists(topk.run_tas_gas_policies(case.t.gen, case.gas_gen, p, ids_t, C, 0,
                                                  *case.gas_t, cand_t=cd))
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_array_equal(got[0], want[0])
            assert got[1].sum() > 0
