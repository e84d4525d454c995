"""Sparse constraints handed over as the CSR of their entries (skf_theta_desc.data == NULL, skf_plan_set_constraint_entries)
against the same constraints handed over dense with a non-zero bound -- the SAME cases on the host emulator and on the GPU.
Both forms hold the same lists after bind, so every iteration must agree bit for bit; hub rows (SKF_THETA_HUB_ROW) are cut
into segments whose partial sums are stored and added in a fixed order."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, DeviceKnownEntries, KnownEntries, launch_count, upload_graph
from oracle import dfmf_oracle as orc
from helpers import relerr, within, DEVIATIONS

VARIANT = {'dfmf': nat.SKF_DFMF, 'dfmc': nat.SKF_DFMC, 'transform': nat.SKF_TRANSFORM}


def entries_of(theta):
    """Dense constraint -> KnownEntries of its non-zero entries (row-major: the lists the device compacts it to)."""
    theta = np.asarray(theta, dtype=np.float64)
    rows, cols = np.nonzero(theta)
    indptr = np.zeros(theta.shape[0] + 1, dtype=np.int64)
    np.cumsum((theta != 0).sum(axis=1), out=indptr[1:])
    return KnownEntries(indptr, cols, theta[rows, cols], theta.shape, unstored='zero')


def pattern_theta(n, seed, per_row=3, empty_row=7):
    """A symmetric pattern of about `per_row` entries per row with both signs, plus a diagonal, plus one empty row."""
    rs = np.random.RandomState(seed)
    th = np.zeros((n, n))
    k = n * per_row // 2
    i, j = rs.randint(0, n, k), rs.randint(0, n, k)
    v = rs.randint(1, 8, k) / 16.0 * np.where(rs.rand(k) < 0.5, -1.0, 1.0)
    th[i, j] = v
    th[j, i] = v
    th[np.arange(n), np.arange(n)] = 0.05
    th[empty_row, :] = 0.0
    th[:, empty_row] = 0.0
    return th


N1 = {'a': 131, 'b': 197, 'c': 70}


def graph1(ranks, seed=0, masked=False):
    """Three types, two relations, constraints on `b` (pattern) and on `a` (lambda I)."""
    rs = np.random.RandomState(seed)
    types = ['a', 'b', 'c']
    M = (rs.rand(N1['a'], N1['b']) < 0.4) if masked else None
    rels = [('a', 'b', rs.rand(N1['a'], N1['b']), M), ('b', 'c', rs.rand(N1['b'], N1['c']), None)]
    thetas = [('b', pattern_theta(N1['b'], seed + 1)), ('a', 0.01 * np.eye(N1['a']))]
    G0 = {t: rs.rand(N1[t], ranks[t]) + 0.05 for t in types}
    return types, rels, thetas, G0


def as_entries(thetas):
    return [(t, entries_of(th)) for t, th in thetas]


def run_plan(variant, types, n, ranks, rels, thetas, G0, dtype, iters, target=None, S=None, engine=None):
    """(factors, backbones, launches of the iterations, workspace bytes, batchable) of one plan."""
    plan = DevicePlan(types, n, ranks, rels, thetas, VARIANT[variant], dtype=dtype, target=target, engine=engine)
    try:
        for t in types:
            plan.set_factor(t, G0[t])
        if S is not None:
            for k, s in enumerate(S):
                plan.set_backbone(k, s)
        before = launch_count()
        plan.iterate(iters)
        launches = launch_count() - before
        G = {t: plan.get_factor(t) for t in types}
        Sout = [plan.get_backbone(k) for k in range(len(rels))]
        return G, Sout, launches, plan.workspace_bytes, plan.batchable()
    finally:
        plan.close()


def same_bits(a, b, what):
    Ga, Sa = a[0], a[1]
    Gb, Sb = b[0], b[1]
    for t in Ga:
        assert np.isfinite(Ga[t]).all(), '%s: G_%s not finite' % (what, t)
        assert np.array_equal(Ga[t], Gb[t]), '%s: G_%s differs' % (what, t)
    for k in range(len(Sa)):
        assert np.array_equal(Sa[k], Sb[k]), '%s: S_%d differs' % (what, k)


def entries_against_dense(variant, dtype, c_b, monkeypatch, general=False, iters=3, engine=None, expect_small=None):
    """Test 1: the graph with Theta dense-fed (ndarray: the host layer counts its non-zeros for the bound) and entries-fed."""
    if general:
        monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    ranks = {'a': 8, 'b': c_b, 'c': 6}
    types, rels, thetas, G0 = graph1(ranks, seed=c_b, masked=variant == 'dfmc')
    target, S = None, None
    if variant == 'transform':             # fold `b` in: the constraint on the target only, frozen factors of a / c, backbones
        target = 'b'
        types = ['b', 'a', 'c']
        thetas = thetas[:1]
        rs = np.random.RandomState(5)
        S = [rs.rand(ranks['a'], ranks['b']), rs.rand(ranks['b'], ranks['c'])]
    dense = run_plan(variant, types, N1, ranks, rels, thetas, G0, dtype, iters, target, S, engine)
    lists = run_plan(variant, types, N1, ranks, rels, as_entries(thetas), G0, dtype, iters, target, S, engine)
    what = '%s %s c_b %d%s' % (variant, dtype, c_b, ' general' if general else '')
    same_bits(lists, dense, what)
    assert lists[2] == dense[2], '%s: %d launches entries-fed, %d dense-fed' % (what, lists[2], dense[2])
    assert lists[4] == dense[4]
    if expect_small is not None:
        assert lists[4] == expect_small, '%s: small-graph schedule %s' % (what, lists[4])
    # no dense form anywhere: the entries-fed workspace is the dense-fed one (whose lists are sized by the same count)
    assert lists[3] <= dense[3]
    return lists


def batch_case(dtype):
    """skf_iterate_batch over 3 restarts of the entries-fed graph (one upload) against one restart after the other."""
    ranks = {'a': 8, 'b': 20, 'c': 6}
    types, rels, thetas, _ = graph1(ranks, seed=3)
    rel_dev, th_dev = upload_graph(rels, as_entries(thetas), dtype)
    assert all(isinstance(d, DeviceKnownEntries) for _, d in th_dev)
    G0s = [{t: np.random.RandomState(10 + k).rand(N1[t], ranks[t]) + 0.05 for t in types} for k in range(3)]
    plans = [DevicePlan(types, N1, ranks, rel_dev, th_dev, nat.SKF_DFMF, dtype=dtype) for _ in range(3)]
    try:
        for p, G0 in zip(plans, G0s):
            assert p.batchable()
            for t in types:
                p.set_factor(t, G0[t])
        assert DevicePlan.iterate_batch(plans, 3)
        nat.get_runtime().mem.synchronize()
        got = [({t: p.get_factor(t) for t in types}, [p.get_backbone(k) for k in range(2)]) for p in plans]
    finally:
        for p in plans:
            p.close()
    for k, G0 in enumerate(G0s):
        one = run_plan('dfmf', types, N1, ranks, rels, thetas, G0, dtype, 3)
        same_bits(got[k], one, 'batched restart %d %s' % (k, dtype))


# ---- test 2: no dense twin on the list path -------------------------------------------------------------------------------
N2 = {'a': 64, 'b': 48}
# Bounds of the entries-fed list pass against the dense-fed dense product of the same engine, 3 iterations (helpers.within).
# GPU: at most 10 x the deviation measured on the MI355X (profiles/r14_theta_csr.txt) -- f32: measured 0 (the dense f32
# product adds a row's terms in ascending column order, as the list pass does, and a zero entry adds nothing), so the bound
# is equality; bf16: measured 7.6e-4 (f32 master rows against bf16 copies of Theta and G).  Emulator (another arithmetic:
# its matrix-core stand-in sums a tile in another order): f32 from the format, 64 terms x 2^-23; bf16 as on the GPU.
HALF_FULL_TOL = {'GPU': {'f32': 0.0, 'bf16': 7e-3}, 'emulator': {'f32': 64 * 2.0 ** -23, 'bf16': 7e-3}}


def half_full_graph(seed=0):
    rs = np.random.RandomState(seed)
    th = np.where(rs.rand(64, 64) < 0.5, (rs.rand(64, 64) - 0.5) / 8.0, 0.0)
    th = (th + th.T) / 2.0
    ranks = {'a': 12, 'b': 8}
    rels = [('a', 'b', rs.rand(64, 48), None)]
    G0 = {t: rs.rand(N2[t], ranks[t]) + 0.05 for t in ('a', 'b')}
    return ['a', 'b'], ranks, rels, th, G0


def half_full_case(dtype, where, iters=3):
    """nnz > n^2 / 16 as entries: kept as lists (no dense form to fall back on), the general schedule."""
    types, ranks, rels, th, G0 = half_full_graph()
    assert np.count_nonzero(th) > 64 * 64 // 16
    lists = run_plan('dfmf', types, N2, ranks, rels, [('a', entries_of(th))], G0, dtype, iters)
    assert not lists[4], 'a constraint denser than n^2 / 16 rides the small-graph schedule'
    if dtype == 'f64':
        Go, So = orc.dfmf({('a', 'b'): [rels[0][2]]}, {('a', 'a'): [th]}, types, ranks, max_iter=iters,
                          G0={(t, t): G0[t] for t in types})
        for t in types:
            assert relerr(lists[0][t], Go[t, t]) < 1e-9
        assert relerr(lists[1][0], So['a', 'b'][0]) < 1e-9
        return
    dense = run_plan('dfmf', types, N2, ranks, rels, [('a', th)], G0, dtype, iters)
    worst = max([relerr(lists[0][t], dense[0][t]) for t in types] + [relerr(lists[1][0], dense[1][0])])
    print('half-full constraint, %s %s: entries-fed vs dense product %.3e' % (where, dtype, worst))
    bound, what = HALF_FULL_TOL[where][dtype], '%s %s: half-full constraint as entries vs the dense product' % (where, dtype)
    if bound == 0.0:
        DEVIATIONS.append((what, worst, 0.0))
        assert worst == 0.0, '%s: measured %.3e, bound: equality' % (what, worst)
    else:
        within(worst, bound, what)


def all_zero_case(dtype, monkeypatch):
    """nnz = 0: the plan of the same graph without the constraint, bit for bit (both on the general schedule)."""
    monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    types, ranks, rels, th, G0 = half_full_graph(1)
    zero = KnownEntries(np.zeros(65, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (64, 64), unstored='zero')
    with_zero = run_plan('dfmf', types, N2, ranks, rels, [('a', zero)], G0, dtype, 3)
    without = run_plan('dfmf', types, N2, ranks, rels, [], G0, dtype, 3)
    same_bits(with_zero, without, 'all-zero constraint %s' % dtype)


# ---- test 3: hub rows ---------------------------------------------------------------------------------------------------
HUB_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 299)


def hub_graph(n, c, lengths, seed=0):
    """`n` objects; the rows hub_rows(n) hold `lengths` entries, the rest about 3.  Values +-m / 8 (m < 8) and G0 = k / 16
    (0 < k < 16): every partial sum of the constraint pass is exact in f32 and f64, whatever the order."""
    rs = np.random.RandomState(seed)
    th = np.zeros((n, n))
    special = hub_rows(n, len(lengths))
    for r in range(n):
        L = lengths[special.index(r)] if r in special else 3
        L = min(L, n)
        cols = rs.choice(n, L, replace=False)
        th[r, cols] = rs.randint(1, 8, L) / 8.0 * np.where(rs.rand(L) < 0.5, -1.0, 1.0)
    ranks = {'b': c, 'p': 4}
    nn = {'b': n, 'p': 40}
    rels = [('b', 'p', rs.randint(0, 16, (n, 40)) / 16.0, None)]
    G0 = {t: rs.randint(1, 16, (nn[t], ranks[t])) / 16.0 for t in ('b', 'p')}
    return ['b', 'p'], nn, ranks, rels, th, G0


def hub_rows(n, count):
    """Rows spread over the whole type, so that they fall on both sides of any boundary between two owners."""
    return [(2 * k + 1) * n // (2 * count) for k in range(count)]


def hub_case(dtype, c, monkeypatch, n=300, lengths=HUB_LENGTHS):
    monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    lengths = tuple(min(L, n - 1) for L in lengths)
    types, nn, ranks, rels, th, G0 = hub_graph(n, c, lengths)
    out = {}
    for hub in ('64', '0'):
        monkeypatch.setenv('SKF_THETA_HUB_ROW', hub)
        out[hub, 'dense'] = run_plan('dfmf', types, nn, ranks, rels, [('b', th)], G0, dtype, 1)
        out[hub, 'lists'] = run_plan('dfmf', types, nn, ranks, rels, [('b', entries_of(th))], G0, dtype, 1)
    what = 'hub rows %s c %d' % (dtype, c)
    same_bits(out['64', 'dense'], out['0', 'dense'], what + ': split vs unsplit')
    same_bits(out['64', 'lists'], out['64', 'dense'], what + ': entries-fed vs dense-fed, split')
    same_bits(out['0', 'lists'], out['0', 'dense'], what + ': entries-fed vs dense-fed, unsplit')
    for form in ('dense', 'lists'):         # the two hub kernels ran, and nothing else changed
        assert out['64', form][2] - out['0', form][2] == 2, (what, form, out['64', form][2], out['0', form][2])
    if dtype == 'f64':
        monkeypatch.setenv('SKF_THETA_HUB_ROW', '64')
        got = run_plan('dfmf', types, nn, ranks, rels, [('b', entries_of(th))], G0, dtype, 3)
        Go, So = orc.dfmf({('b', 'p'): [rels[0][2]]}, {('b', 'b'): [th]}, types, ranks, max_iter=3,
                          G0={(t, t): G0[t] for t in types})
        for t in types:
            assert relerr(got[0][t], Go[t, t]) < 1e-9
        assert relerr(got[1][0], So['b', 'p'][0]) < 1e-9


def hub_owned_case(monkeypatch, c=65, n=300):
    """Two owners of rows, dense-fed (entries-fed constraints are refused there): the hub rows on both sides of the boundary;
    f64 within the bound of test_owned_sharding.py (1e-9) of the single-device result."""
    from helpers import fit_owned
    monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    monkeypatch.setenv('SKF_THETA_HUB_ROW', '64')
    types, nn, ranks, rels, th, G0 = hub_graph(n, c, HUB_LENGTHS)
    rows = hub_rows(n, len(HUB_LENGTHS))
    assert min(rows) < n // 2 - 64 and max(rows) > n // 2 + 64
    single = run_plan('dfmf', types, nn, ranks, rels, [('b', th)], G0, 'f64', 3)
    R = {('b', 'p'): [rels[0][2]]}
    out, _, _ = fit_owned('dfmf', R, None, {('b', 'b'): [th]}, types, ranks, {(t, t): G0[t] for t in types}, 3, 2)
    for G, S in out:
        for t in types:
            assert relerr(G[t, t], single[0][t]) < 1e-9
        assert relerr(S['b', 'p'][0], single[1][0]) < 1e-9


# ---- test 4: refusals -----------------------------------------------------------------------------------------------------
def small_constraint(which):
    """Six entries of a constraint on 4 objects: canonical ('ok') or broken in one of the ways bind refuses."""
    indptr = np.array([0, 2, 4, 4, 6], dtype=np.int64)
    idx = np.array([1, 3, 0, 2, 0, 3], dtype=np.int32)
    nnz = 6
    if which == 'first':
        indptr[0] = 1
    elif which == 'last':
        nnz = 7                                         # indptr[n] != nnz
    elif which == 'step':
        indptr[2] = 1                                   # 2 -> 1 -> 4: a negative step
    elif which == 'range':
        idx[3] = 4                                      # column 4 of 4
    elif which == 'negative':
        idx[2] = -1
    elif which == 'order':
        idx[2], idx[3] = 2, 0
    elif which == 'equal':
        idx[1] = 1                                      # 1, 1: not STRICTLY ascending
    else:
        assert which in ('ok', 'handover')
    return indptr, idx, nnz


BROKEN = ('first', 'last', 'step', 'range', 'negative', 'order', 'equal')


def raw_plan(which, dtype='f64', variant=nat.SKF_DFMF):
    """A plan created through the C ABI (no host-side check in the way): types a (4 objects, the constraint) and b (6), one
    dense relation.  Returns (runtime, handle, keep-alive list, workspace-to-be)."""
    rt = nat.get_runtime()
    mem = rt.mem
    code = nat.DTYPES[dtype]
    npd = nat.NP_DTYPE[code]
    indptr, idx, nnz = small_constraint(which)
    keep = [mem.from_host(indptr), mem.from_host(idx), mem.from_host(np.full(8, 0.25, dtype=npd)),
            mem.from_host(np.random.RandomState(0).rand(4, 6).astype(npd))]
    tdesc = (nat.TypeDesc * 2)()
    tdesc[0].n_obj, tdesc[0].rank, tdesc[1].n_obj, tdesc[1].rank = 4, 2, 6, 2
    rdesc = (nat.RelationDesc * 1)()
    rdesc[0].row_type, rdesc[0].col_type, rdesc[0].data, rdesc[0].ld = 0, 1, keep[3].ptr, 6
    if code == nat.SKF_BF16:
        keep[3] = mem.from_host(nat.to_bf16_bits(np.random.RandomState(0).rand(4, 6).astype(np.float32)))
        rdesc[0].data = keep[3].ptr
    hdesc = (nat.ThetaDesc * 1)()
    hdesc[0].type, hdesc[0].data, hdesc[0].ld, hdesc[0].nnz = 0, None, 0, nnz
    opt = nat.Options(code, variant, 0 if variant == nat.SKF_TRANSFORM else -1, nat.SKF_ENGINE_MFMA, 0, 0, 0)
    handle = nat._P()
    rt.call('skf_plan_create', 2, tdesc, 1, rdesc, 1, hdesc, C.byref(opt), C.byref(handle))
    return rt, handle, keep


def bind(rt, handle, keep):
    nbytes = C.c_size_t()
    rt.call('skf_plan_workspace_bytes', handle, C.byref(nbytes))
    ws = rt.mem.empty(nbytes.value)
    keep.append(ws)
    rt.call('skf_plan_bind_workspace', handle, ws.ptr, nbytes.value, rt.mem.stream)


def refusal_case(which, dtype='f64'):
    """A broken list is SKF_E_INVALID at bind after exactly ONE launch -- the validation, nothing that gathers through the
    lists -- with a message naming the constraint; a missing hand-over is refused before any launch."""
    rt, handle, keep = raw_plan(which, dtype)
    try:
        if which != 'handover':
            rt.call('skf_plan_set_constraint_entries', handle, 0, keep[0].ptr, keep[1].ptr, keep[2].ptr)
        before = launch_count()
        if which == 'ok':
            bind(rt, handle, keep)
            return
        with pytest.raises(nat.SkfNativeError) as err:
            bind(rt, handle, keep)
        assert err.value.code == nat.SKF_E_INVALID
        assert 'constraint 0' in str(err.value)
        if dtype != 'bf16':         # (SKF_BF16 converts the relations first: launches that read no list of the constraint)
            assert launch_count() - before == (0 if which == 'handover' else 1)
    finally:
        rt.lib.skf_plan_destroy(handle)


def setter_state_case():
    """The setter after bind is SKF_E_STATE; a constraint index out of range, a dense-fed constraint and null lists are
    SKF_E_INVALID."""
    rt, handle, keep = raw_plan('ok')
    try:
        for bad in (-1, 1):
            with pytest.raises(nat.SkfNativeError) as err:
                rt.call('skf_plan_set_constraint_entries', handle, bad, keep[0].ptr, keep[1].ptr, keep[2].ptr)
            assert err.value.code == nat.SKF_E_INVALID and 'out of range' in str(err.value)
        with pytest.raises(nat.SkfNativeError) as err:
            rt.call('skf_plan_set_constraint_entries', handle, 0, None, keep[1].ptr, keep[2].ptr)
        assert err.value.code == nat.SKF_E_INVALID
        rt.call('skf_plan_set_constraint_entries', handle, 0, keep[0].ptr, keep[1].ptr, keep[2].ptr)
        bind(rt, handle, keep)
        with pytest.raises(nat.SkfNativeError) as err:
            rt.call('skf_plan_set_constraint_entries', handle, 0, keep[0].ptr, keep[1].ptr, keep[2].ptr)
        assert err.value.code == nat.SKF_E_STATE
    finally:
        rt.lib.skf_plan_destroy(handle)
    # a constraint with a dense form takes no entries
    plan = DevicePlan(['a', 'b'], {'a': 4, 'b': 6}, {'a': 2, 'b': 2}, [('a', 'b', np.ones((4, 6)), None)],
                      [('a', np.eye(4))], nat.SKF_DFMF)
    try:
        with pytest.raises(nat.SkfNativeError) as err:
            rt.call('skf_plan_set_constraint_entries', plan.handle, 0, keep[0].ptr, keep[1].ptr, keep[2].ptr)
        assert err.value.code in (nat.SKF_E_INVALID, nat.SKF_E_STATE)
    finally:
        plan.close()
    assert rt.lib.skf_abi_version() == nat.SKF_ABI_VERSION == 5


def create_status(lib, nnz, variant=nat.SKF_DFMF, n_rows=0, part=(0, 0), flags=0, theta_type=0, keep=None):
    """Status of skf_plan_create for 40 x 30 objects, one dense relation and one constraint given as its entries (no HIP
    call is made before the validation answers; `keep`: any readable address for the relation's data pointer)."""
    tdesc = (nat.TypeDesc * 2)()
    tdesc[0].n_obj, tdesc[0].rank, tdesc[1].n_obj, tdesc[1].rank = 40, 8, 30, 6
    rdesc = (nat.RelationDesc * 1)()
    rdesc[0].row_type, rdesc[0].col_type, rdesc[0].data, rdesc[0].ld = 0, 1, keep, 30
    rdesc[0].n_rows = n_rows
    hdesc = (nat.ThetaDesc * 1)()
    hdesc[0].type, hdesc[0].data, hdesc[0].ld, hdesc[0].nnz = theta_type, None, 0, nnz
    opt = nat.Options(nat.SKF_F64, variant, 0 if variant == nat.SKF_TRANSFORM else -1, nat.SKF_ENGINE_MFMA, part[0], part[1], flags)
    handle = nat._P()
    try:
        return lib.skf_plan_create(2, tdesc, 1, rdesc, 1, hdesc, C.byref(opt), C.byref(handle))
    finally:
        if handle.value:
            lib.skf_plan_destroy(handle)


def creation_cases(lib, keep):
    """Refused at skf_plan_create, before any HIP call: row blocks, slices, owned rows, a negative count, more than 2e9."""
    bad = nat.SKF_E_INVALID
    assert create_status(lib, 10, keep=keep) == 0
    assert create_status(lib, 0, keep=keep) == 0                                        # an all-zero constraint
    assert create_status(lib, 1600, keep=keep) == 0                                     # full: lists whatever the density
    assert create_status(lib, 10, nat.SKF_DFMC, keep=keep) == 0
    assert create_status(lib, 10, nat.SKF_TRANSFORM, keep=keep) == 0                    # on the target
    assert create_status(lib, 10, nat.SKF_TRANSFORM, theta_type=1, keep=keep) == bad    # ... only
    assert create_status(lib, 10, n_rows=20, keep=keep) == bad                          # a row block
    assert b'constraint 0' in lib.skf_last_error()
    assert create_status(lib, 10, part=(0, 2), keep=keep) == bad                        # a sliced plan
    assert b'constraint 0' in lib.skf_last_error()
    assert create_status(lib, 10, part=(0, 2), flags=nat.SKF_OPT_OWNED_ROWS, n_rows=20, keep=keep) == bad
    assert create_status(lib, 10, part=(0, 1), flags=nat.SKF_OPT_OWNED_ROWS, keep=keep) == bad
    assert b'constraint 0' in lib.skf_last_error()
    assert create_status(lib, -1, keep=keep) == bad
    assert create_status(lib, 2000000001, keep=keep) == bad
    assert b'2e9' in lib.skf_last_error()
    assert create_status(lib, 10, theta_type=2, keep=keep) == bad                       # a type out of range
    assert lib.skf_abi_version() == 5


# ---- test 5: the public API --------------------------------------------------------------------------------------------
def api_theta(n, seed, per_row=2):
    """A scipy COO constraint with a duplicate pair (summed) and an explicit zero, symmetric, both signs, a diagonal."""
    th = pattern_theta(n, seed, per_row)
    coo = scipy.sparse.coo_matrix(th)
    r = np.concatenate([coo.row, [1, 1, 2]])
    c = np.concatenate([coo.col, [0, 0, 5]])
    v = np.concatenate([coo.data, [0.125, 0.0625, 0.0]])
    dense = th.copy()
    dense[1, 0] += 0.1875
    return scipy.sparse.coo_matrix((v, (r, c)), shape=(n, n)), dense


def api_graph(theta, n=(60, 45), ranks=(6, 5), seed=0, **kw):
    from skfusion_amd.fusion import FusionGraph, Relation, ObjectType
    rs = np.random.RandomState(seed)
    t1, t2 = ObjectType('t1', ranks[0]), ObjectType('t2', ranks[1])
    return FusionGraph([Relation(rs.rand(n[0], n[1]), t1, t2, name='r'), Relation(theta, t1, t1, name='theta', **kw)])


def forbid(monkeypatch, sp):
    from sparse_dfmf_api_cases import forbid_toarray
    return forbid_toarray(monkeypatch, sp)


def fit_factors(fit):
    g = fit.fusion_graph
    types = sorted(g.object_types, key=lambda t: t.name)
    rel = [r for r in g.relations if r.row_type != r.col_type][0]
    return [np.asarray(f) for t in types for f in fit.factors_[t]] + [np.asarray(s) for s in fit.backbones_[rel]]


def same_fits(a, b, what):
    fa, fb = fit_factors(a), fit_factors(b)
    assert len(fa) == len(fb)
    for x, y in zip(fa, fb):
        assert np.isfinite(x).all()
        assert np.array_equal(x, y), what


def api_constraint_entries_case(monkeypatch):
    """Relation.constraint_entries(): csr / csc / coo with duplicates and explicit zeros -> the lists of the dense matrix."""
    from skfusion_amd.fusion import Relation, ObjectType
    coo, dense = api_theta(60, 2)
    want = entries_of(dense)
    t = ObjectType('t', 4)
    for fmt in ('csr', 'csc', 'coo'):
        sp = forbid(monkeypatch, coo.asformat(fmt))
        ke = Relation(sp, t, t).constraint_entries()
        assert ke.unstored == 'zero' and not ke.by_col and ke.shape == (60, 60)
        assert ke.indptr.tobytes() == want.indptr.tobytes(), fmt
        assert ke.indices.tobytes() == want.indices.tobytes(), fmt
        assert ke.values.tobytes() == want.values.tobytes(), fmt
        ke.validate()


def api_fit_case(cls_name, dtype, monkeypatch, **kw):
    """Dfmf / Dfmc: the scipy.sparse constraint (never toarray()) gives the factors of the dense ndarray constraint."""
    import skfusion_amd.fusion as F
    cls = getattr(F, cls_name)
    coo, dense = api_theta(60, 3)
    args = dict(max_iter=3, init_type='random', random_state=1, dtype=dtype, **kw)
    assert coo.tocsr().nnz <= 60 * 60 // 16                    # (sparse by the default rule)
    for fmt in ('csr', 'csc', 'coo'):
        a = cls(**args).fuse(api_graph(forbid(monkeypatch, coo.asformat(fmt))))
        b = cls(**args).fuse(api_graph(dense))
        same_fits(a, b, '%s %s %s' % (cls_name, dtype, fmt))


def api_transform_case(dtype, monkeypatch, n_run=1):
    """DfmfTransform: new objects of t1 with a sparse constraint on them against the dense ndarray constraint."""
    from skfusion_amd.fusion import Dfmf, DfmfTransform, FusionGraph, Relation
    coo, dense = api_theta(60, 4)
    fuser = Dfmf(max_iter=3, init_type='random', random_state=0, dtype=dtype, n_run=n_run).fuse(api_graph(dense))
    t1, t2 = sorted(fuser.fusion_graph.object_types, key=lambda t: t.name)
    new_coo, new_dense = api_theta(48, 5, per_row=1)
    assert new_coo.tocsr().nnz <= 48 * 48 // 16                # (sparse by the default rule)
    new_R = np.random.RandomState(3).rand(48, 45)
    out = []
    for theta in (forbid(monkeypatch, new_coo.tocsr()), new_dense):
        g = FusionGraph([Relation(new_R, t1, t2), Relation(theta, t1, t1)])
        tr = DfmfTransform(max_iter=3, init_type='random', random_state=2, dtype=dtype, n_run=n_run).transform(t1, g, fuser)
        out.append([np.asarray(tr.factor(t1, run)) for run in range(n_run)])
    for x, y in zip(*out):
        assert x.shape == (48, 6) and np.isfinite(x).all()
        assert np.array_equal(x, y), 'fold-in %s' % dtype


def expanded(sp_graph, fuser):
    """Whether the fuser expands the graph's constraint (True) or hands its entries over (False)."""
    from skfusion_amd.fusion.decomposition import dfmf as dfmf_mod
    _, Theta = dfmf_mod.graph_matrices(sp_graph, shard=fuser.shard, sparse_constraints=fuser.sparse_constraints)
    kinds = [isinstance(m, KnownEntries) for mats in Theta.values() for m in mats]
    assert len(kinds) == 1
    return not kinds[0]


def api_rule_case(monkeypatch):
    """sparse_constraints False / None / True, the n^2 / 16 rule, shard != 'runs', unstored='unknown', a preprocessor."""
    from skfusion_amd.fusion import Dfmf, Dfmc
    coo, dense = api_theta(60, 6)
    base = dict(max_iter=2, init_type='random', random_state=1)
    sparse_g = api_graph(coo.tocsr())
    rs = np.random.RandomState(0)
    full = scipy.sparse.csr_matrix(np.where(rs.rand(60, 60) < 0.5, 0.25, 0.0))              # nnz > n^2 / 16
    assert full.nnz > 60 * 60 // 16 >= coo.tocsr().nnz
    for cls in (Dfmf, Dfmc):
        assert not expanded(sparse_g, cls(**base))
        assert not expanded(sparse_g, cls(sparse_constraints=True, **base))
        assert expanded(sparse_g, cls(sparse_constraints=False, **base))
        assert expanded(api_graph(full), cls(**base))
        assert not expanded(api_graph(full), cls(sparse_constraints=True, **base))
        assert expanded(sparse_g, cls(shard='relations', sparse_constraints=True, **base))
        assert expanded(api_graph(coo.tocsr(), unstored='unknown'), cls(sparse_constraints=True, **base))
        assert expanded(api_graph(coo.tocsr(), preprocessor=lambda x: x), cls(sparse_constraints=True, **base))
    # expanding is what happened before: toarray() is called, the result is the dense one
    calls = []
    sp = coo.tocsr()
    orig = sp.toarray
    monkeypatch.setattr(sp, 'toarray', lambda *a, **k: (calls.append(1), orig(*a, **k))[1], raising=False)
    a = Dfmf(sparse_constraints=False, **base).fuse(api_graph(sp))
    assert calls
    same_fits(a, Dfmf(**base).fuse(api_graph(dense)), 'sparse_constraints=False')
    # the dense one by the rule takes the dense product: the result of its ndarray, bit for bit; forced to lists: close
    a = Dfmf(**base).fuse(api_graph(full))
    b = Dfmf(**base).fuse(api_graph(full.toarray()))
    same_fits(a, b, 'dense by the rule')
    c = Dfmf(sparse_constraints=True, **base).fuse(api_graph(forbid(monkeypatch, full.copy())))
    for x, y in zip(fit_factors(c), fit_factors(b)):
        assert relerr(x, y) < 1e-9
    # the functional seams refuse entries in a sharded fit (the class layer never sends them there)
    from skfusion_amd.fusion.decomposition import _dfmf, _dfmc
    R = {('a', 'b'): [np.ones((4, 6))]}
    Theta = {('a', 'a'): [entries_of(np.eye(4))]}
    for shard in ('relations', 'rows', 'owned'):
        with pytest.raises(ValueError, match='entries'):
            _dfmf.dfmf(R, Theta, ['a', 'b'], {'a': 2, 'b': 2}, max_iter=1, shard=shard)
        with pytest.raises(ValueError, match='entries'):
            _dfmc.dfmc(R, {('a', 'b'): [None]}, Theta, ['a', 'b'], {'a': 2, 'b': 2}, max_iter=1, shard=shard)


def api_restarts_case(dtype, monkeypatch):
    """n_run=3 (restarts of a small graph share their launches and ONE upload) equals three single runs; the shared-launch
    rule counts the constraint's non-zeros on the sparse matrix."""
    from skfusion_amd.fusion import Dfmf
    from skfusion_amd.fusion.decomposition import dfmf as dfmf_mod
    coo, dense = api_theta(60, 7)
    kw = dict(max_iter=3, init_type='random', dtype=dtype)
    g3 = api_graph(forbid(monkeypatch, coo.tocsr()))
    f3 = Dfmf(n_run=3, random_state=4, **kw)
    f3.fusion_graph = g3
    assert dfmf_mod.shared_launches(f3)
    f3.fuse(g3)
    rs = np.random.RandomState(4)
    t1, t2 = sorted(g3.object_types, key=lambda t: t.name)
    rel = [r for r in g3.relations if r.row_type != r.col_type][0]
    for run in range(3):
        one = Dfmf(n_run=1, random_state=rs, **kw).fuse(api_graph(dense))
        o1, o2 = sorted(one.fusion_graph.object_types, key=lambda t: t.name)
        assert np.array_equal(f3.factors_[t1][run], one.factors_[o1][0]), 'run %d' % run
        assert np.array_equal(f3.factors_[t2][run], one.factors_[o2][0]), 'run %d' % run
        orel = [r for r in one.fusion_graph.relations if r.row_type != r.col_type][0]
        assert np.array_equal(f3.backbones_[rel][run], one.backbones_[orel][0]), 'run %d' % run


def api_save_load_case(tmp_path, monkeypatch):
    from skfusion_amd.fusion import Dfmf
    from skfusion_amd.fusion.base import FusionFit
    coo, _ = api_theta(60, 8)
    g = api_graph(forbid(monkeypatch, coo.tocsr()))
    f = Dfmf(max_iter=2, init_type='random', random_state=2).fuse(g)
    rel = [r for r in g.relations if r.row_type != r.col_type][0]
    path = f.save(str(tmp_path / 'fit.npz'))
    loaded = FusionFit.load(path, g)
    assert np.array_equal(loaded.complete(rel), f.complete(rel))
    for t in g.object_types:
        assert np.array_equal(loaded.factor(t), f.factor(t))
