"""The column-mean initialisers `random_c` / `random_vcol` on the device (csrc/skf_init.h, skf_plan_relation_norms,
skf_plan_init_column_means, DevicePlan.relation_norms / init_column_means, `init_device` of Dfmf / Dfmc) against the host
initialiser `_init.initialize` -- shared by the emulator (a subset) and the GPU tests.

The graph of every plan-level case: types a, b, c with the relations (a, b) and (b, c), so that b is touched by two views
-- the transpose of the first relation, then the second as it is -- and their order matters.

1. exact data (0/1 entries, ratings 0 .. 5; every partial sum below 2^24, the data exact in bf16): byte for byte
2. uniform random f64 data under the bound  |G_dev - G_host| <= sum over views 2 take u mean|v| + 4 u |G|
   (u = 2^-53 / 2^-24: the host's pairwise sum and any device order of the `take` terms both lie within
   take u sum|v| / take of the true mean; the f32 engine's rounding of the data is one more u mean|v|, and take >= 1;
   4 u |G| covers the additions of the views and the final rounding) -- checked in float64 against the product form first
3. refusals before any write, guard bands, padding of a strided output
4. the public API: init_device=True equals init_device=False byte for byte on exact data."""
import ctypes as C

import numpy as np
import scipy.sparse

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, KnownEntries
from skfusion_amd.fusion.decomposition import _init

TYPES = ['a', 'b', 'c']
U = {'f64': 2.0 ** -53, 'f32': 2.0 ** -24}


# ---- data ----------------------------------------------------------------------------------------------------------------------
def exact_relation(shape, kind, seed):
    """kind 'ratings': 0 on two thirds of the cells, 1 .. 5 elsewhere; 'binary': 0/1 at one cell in four (columns tie
    heavily either way); 'ones': 0/1 at one cell in 400 (what SKF_BF16 keeps as lists of its ones beside the bitmap)."""
    rs = np.random.RandomState(seed)
    if kind == 'ratings':
        return np.where(rs.rand(*shape) < 1.0 / 3.0, np.floor(rs.rand(*shape) * 5.0) + 1.0, 0.0)
    return (rs.rand(*shape) < (0.25 if kind == 'binary' else 0.0025)).astype(np.float64)


def relations(sizes, kind, form, seed=3, real=False):
    """(host dict R_first, rel_list for DevicePlan): `form` 'dense' | 'csr' (the stored entries, unstored = zero)."""
    host, rels = {}, []
    for q, (i, j) in enumerate((('a', 'b'), ('b', 'c'))):
        shape = (sizes[TYPES.index(i)], sizes[TYPES.index(j)])
        m = np.random.RandomState(seed + q).rand(*shape) if real else exact_relation(shape, kind, seed + q)
        host[i, j] = m
        if form == 'csr':
            s = scipy.sparse.csr_matrix(m)
            rels.append((i, j, KnownEntries(s.indptr, s.indices, s.data, s.shape, unstored='zero'), None))
        else:
            rels.append((i, j, m, None))
    return host, rels


def make_plan(sizes, ranks, rels, dtype, variant=nat.SKF_DFMF):
    n_obj = dict(zip(TYPES, sizes))
    rank = dict(zip(TYPES, ranks))
    return DevicePlan(TYPES, n_obj, rank, rels, [], variant, dtype=dtype), n_obj, rank


def device_init(plan, n_obj, rank, host, init_type, seed):
    """(G per type as float64, pools, the RandomState after the draws) of the device initialiser."""
    rs = np.random.RandomState(seed)
    shapes = {k: v.shape for k, v in host.items()}
    di = _init.DeviceInit(_init.draw_positions(TYPES, rank, shapes, init_type, rs), init_type, {})
    di.apply(plan, TYPES)
    return {t: plan.get_factor(t) for t in TYPES}, di.pools, rs


def host_init(n_obj, rank, host, init_type, seed):
    rs = np.random.RandomState(seed)
    pools = {}
    G = _init.initialize(TYPES, n_obj, rank, host, init_type, rs, pools)
    return {t: G[t, t] for t in TYPES}, pools, rs


# ---- 1. exact data ---------------------------------------------------------------------------------------------------------------
def exact_case(dtype, sizes, ranks, kind, form, init_type, seed=5):
    host, rels = relations(sizes, kind, form)
    plan, n_obj, rank = make_plan(sizes, ranks, rels, dtype)
    try:
        got, pools, rs_d = device_init(plan, n_obj, rank, host, init_type, seed)
        want, hpools, rs_h = host_init(n_obj, rank, host, init_type, seed)
        npd = nat.NP_DTYPE[nat.DTYPES[dtype]]
        for t in TYPES:
            up = want[t].astype(npd).astype(np.float64)         # the upload's cast to the master type
            assert got[t].shape == up.shape
            assert got[t].tobytes() == up.tobytes(), 'factor of %s differs from _init.initialize (%s %s %s %s)' % (t, dtype, kind, form, init_type)
        if init_type == 'random_c':
            assert sorted(pools) == sorted(hpools)
            for key in hpools:
                assert np.array_equal(pools[key], np.asarray(hpools[key])), 'pool of view %r' % (key,)
        assert rs_d.randint(1 << 30) == rs_h.randint(1 << 30), 'the random stream was consumed differently'
    finally:
        plan.close()


def norms_case(dtype, sizes, kind, form):
    host, rels = relations(sizes, kind, form)
    plan, _, _ = make_plan(sizes, (5, 7, 5), rels, dtype)
    try:
        for k, key in enumerate((('a', 'b'), ('b', 'c'))):
            rs, cs = plan.relation_norms(k)
            sq = host[key] ** 2
            assert rs.tobytes() == sq.sum(axis=1).tobytes() and cs.tobytes() == sq.sum(axis=0).tobytes(), (dtype, kind, form, key)
            again = plan.relation_norms(k)
            assert again[0].tobytes() == rs.tobytes() and again[1].tobytes() == cs.tobytes()
    finally:
        plan.close()


# ---- 2. real-valued data -----------------------------------------------------------------------------------------------------
def product_form(n_obj, rank, host, init_type, seed, pools):
    """(G, B) in float64: the product form 1e-5 + sum |V W| / take with the draws of `draw_positions`, and per type
    B = sum over the views of 2 take mean|v| (the bound is u B + 4 u |G|)."""
    rs = np.random.RandomState(seed)
    shapes = {k: v.shape for k, v in host.items()}
    pos = _init.draw_positions(TYPES, rank, shapes, init_type, rs)
    G, B = {}, {}
    for t in TYPES:
        acc = np.full((n_obj[t], rank[t]), 1e-5)
        b = np.zeros((n_obj[t], rank[t]))
        for (pair, tr), p in pos[t]:
            V = host[pair].T if tr else host[pair]
            sel = np.asarray(pools[pair, tr])[p] if init_type == 'random_c' else p
            take = sel.shape[1]
            W = np.zeros((V.shape[1], rank[t]))
            for k in range(rank[t]):
                W[sel[k], k] = 1.0
            acc += np.abs(np.dot(V, W) / take)
            b += 2.0 * take * np.dot(np.abs(V), W) / take
        G[t], B[t] = acc, b
    return G, B


def distinct_norms(host):
    """The precondition of `random_c` on real data: adjacent sorted column norms of every view differ by more than 1e-9
    relative, so that sums in another order rank the columns alike."""
    for m in host.values():
        for V in (m, m.T):
            n = np.sort(np.sqrt((V ** 2).sum(axis=0)))
            assert (np.diff(n) > 1e-9 * n[1:]).all()


def bound_on_cpu_case(sizes, ranks, init_type, seed=9):
    """The bound, before anything relies on it: host initialiser against the product form, both float64."""
    host, _ = relations(sizes, None, 'dense', real=True)
    n_obj, rank = dict(zip(TYPES, sizes)), dict(zip(TYPES, ranks))
    distinct_norms(host)
    want, hpools, _ = host_init(n_obj, rank, host, init_type, seed)
    G, B = product_form(n_obj, rank, host, init_type, seed, hpools)
    for t in TYPES:
        assert (np.abs(G[t] - want[t]) <= U['f64'] * B[t] + 4 * U['f64'] * np.abs(want[t])).all()


def real_case(dtype, sizes, ranks, form, init_type, seed=9):
    host, rels = relations(sizes, None, form, real=True)
    # the reference reads the relation the plan holds: the upload's cast to the master type (the ranking of `random_c` by
    # norms that differ in the ninth digit must not hinge on the rounding of the data)
    npd = nat.NP_DTYPE[nat.DTYPES[dtype]]
    host = {k: v.astype(npd).astype(np.float64) for k, v in host.items()}
    distinct_norms(host)
    plan, n_obj, rank = make_plan(sizes, ranks, rels, dtype)
    try:
        got, pools, _ = device_init(plan, n_obj, rank, host, init_type, seed)
        want, hpools, _ = host_init(n_obj, rank, host, init_type, seed)
        if init_type == 'random_c':
            for key in hpools:
                assert np.array_equal(pools[key], np.asarray(hpools[key])), 'pool of view %r' % (key,)
        _, B = product_form(n_obj, rank, host, init_type, seed, hpools)
        worst = 0.0
        for t in TYPES:
            bound = U[dtype] * B[t] + 4 * U[dtype] * np.abs(want[t])
            dev = np.abs(got[t] - want[t])
            worst = max(worst, float((dev / bound).max()))
            assert (dev <= bound).all(), 'factor of %s: %.3g of its bound (%s %s %s)' % (t, (dev / bound).max(), dtype, form, init_type)
        print('init_device real %s %s %s %r %r: worst deviation / bound %.3f' % (dtype, form, init_type, sizes, ranks, worst))
    finally:
        plan.close()


# ---- 3. refusals and guards ----------------------------------------------------------------------------------------------------
class Raw(object):
    """One type of a plan through the C entry points, every buffer the test's own and filled with a pattern."""

    def __init__(self, plan, t, views, ld=None):
        self.plan, self.rt, self.k = plan, plan.rt, plan.index[t]
        self.n, self.c = plan.n_obj[self.k], plan.rank[self.k]
        self.ld = ld or self.c
        mem = self.rt.mem
        self.desc = (nat.InitView * len(views))()
        self.sel = []
        for v, (rel, sel) in enumerate(views):
            s = np.ascontiguousarray(sel, dtype=np.int32)
            self.sel.append(mem.from_host(s if s.size else np.zeros(1, dtype=np.int32)))
            self.desc[v].rel, self.desc[v].take, self.desc[v].sel = rel, s.shape[1], self.sel[-1].ptr
        self.nv = len(views)
        self.item = np.dtype(plan.np_dtype).itemsize
        self.g_pat = np.full(self.n * self.ld * self.item, 0x5A, dtype=np.uint8)
        self.g0 = mem.from_host(self.g_pat)

    def need(self):
        need = C.c_size_t()
        self.rt.call('skf_plan_init_column_means_workspace_bytes', self.plan.handle, self.k, self.nv, self.desc, C.byref(need))
        return need.value

    def scratch(self, nbytes):
        self.ws_pat = np.full(max(nbytes, 1), 0x3C, dtype=np.uint8)
        self.ws = self.rt.mem.from_host(self.ws_pat)
        return self.ws

    def call(self, ws_bytes=None, ws=True):
        rc = self.rt.lib.skf_plan_init_column_means(self.plan.handle, self.k, self.nv, self.desc, self.g0.ptr, self.ld,
                                                    self.ws.ptr if ws else None, len(self.ws_pat) if ws_bytes is None else ws_bytes,
                                                    self.plan.stream)
        self.rt.mem.synchronize()
        return rc

    def untouched(self):
        mem = self.rt.mem
        return (mem.to_host(self.g0, self.g_pat.shape, np.uint8).tobytes() == self.g_pat.tobytes() and
                mem.to_host(self.ws, self.ws_pat.shape, np.uint8).tobytes() == self.ws_pat.tobytes())

    def result(self):
        return self.rt.mem.to_host(self.g0, (self.n, self.ld), self.plan.np_dtype)


def refusals_case(dtype='f32'):
    """Everything refused before any write; a strided output keeps its padding.  Runs under guard bands."""
    from guarded import guarded
    from skfusion_amd.fusion.decomposition._dfmf import owned_plan
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    sizes, ranks = (67, 131, 40), (5, 7, 5)
    host, rels = relations(sizes, 'ratings', 'dense')
    with guarded():
        plan, n_obj, rank = make_plan(sizes, ranks, rels, dtype)
        masked = [(i, j, m, (m == 0) if q == 0 else None) for q, (i, j, m, _) in enumerate(rels)]
        plan_m, _, _ = make_plan(sizes, ranks, masked, dtype, variant=nat.SKF_DFMC)
        plan_o = owned_plan(nat.SKF_DFMF, rels, [], TYPES, n_obj, rank, dtype, None, 0, 1)
        try:
            rs = np.random.RandomState(1)
            good = lambda m, c, take: np.stack([rs.permutation(m)[:take] for _ in range(c)])
            views_b = [(0, good(67, 7, 13)), (1, good(40, 7, 8))]
            # an index out of range, in the last view: found on the device before anything is written
            for bad in (40, -1):
                v = [(0, views_b[0][1]), (1, views_b[1][1].copy())]
                v[1][1][6, 7] = bad
                raw = Raw(plan, 'b', v)
                raw.scratch(raw.need())
                assert raw.call() == INV and b'outside its view' in raw.rt.lib.skf_last_error() and raw.untouched(), bad
            # take == 0 (fewer than 5 columns), and more columns than the view has
            for take in (0, 68):
                raw = Raw(plan, 'b', [(0, np.zeros((7, take), dtype=np.int32)), views_b[1]])
                raw.scratch(1 << 16)
                assert raw.call() == INV and raw.untouched(), take
            # a relation that does not touch the type; a relation index out of range
            for rel in (1, 2, -1):
                raw = Raw(plan, 'a', [(rel, good(131, 5, 26))])
                raw.scratch(1 << 16)
                assert raw.call() == INV and raw.untouched(), rel
            # an uncovered form (a masked relation of a DFMC plan) and a plan with owned rows: the norms refuse as well
            for p in (plan_m, plan_o):
                raw = Raw(p, 'a', [(0, good(131, 5, 26))])
                raw.scratch(1 << 16)
                assert raw.call() == INV and raw.untouched()
                need = C.c_size_t()
                assert raw.rt.lib.skf_plan_init_column_means_workspace_bytes(p.handle, 0, 1, raw.desc, C.byref(need)) == INV
                assert raw.rt.lib.skf_plan_relation_norms(p.handle, 0, raw.g0.ptr, None, raw.ws.ptr, 1 << 16, p.stream) == INV
                assert raw.untouched()
            # (the unmasked relation of the DFMC plan is covered)
            raw = Raw(plan_m, 'c', [(1, good(131, 5, 26))])
            raw.scratch(raw.need())
            assert raw.call() == 0
            # a short, a missing and a misaligned scratch; ld < c; a null output
            raw = Raw(plan, 'b', views_b)
            nb = raw.need()
            raw.scratch(nb + 256)
            assert raw.call(ws_bytes=nb - 1) == WS and raw.call(ws=False) == WS and raw.untouched()
            assert raw.rt.lib.skf_plan_init_column_means(plan.handle, raw.k, 2, raw.desc, raw.g0.ptr, 7, raw.ws.ptr + 8, nb, plan.stream) == WS
            assert raw.rt.lib.skf_plan_init_column_means(plan.handle, raw.k, 2, raw.desc, raw.g0.ptr, 6, raw.ws.ptr, nb, plan.stream) == INV
            assert raw.rt.lib.skf_plan_init_column_means(plan.handle, raw.k, 2, raw.desc, None, 7, raw.ws.ptr, nb, plan.stream) == INV
            assert raw.untouched()
            # ld > c: the padding of every row stays; the values are those of the packed call
            packed = Raw(plan, 'b', views_b)
            packed.scratch(nb)
            assert packed.call() == 0
            wide = Raw(plan, 'b', views_b, ld=10)
            wide.scratch(nb)
            assert wide.call() == 0
            got = wide.result()
            assert got[:, :7].tobytes() == packed.result().tobytes()
            assert got[:, 7:].tobytes() == wide.g_pat.view(plan.np_dtype).reshape(131, 10)[:, 7:].tobytes()
            # the binding refuses a column chosen twice for one factor column
            twice = views_b[0][1].copy()
            twice[3, 5] = twice[3, 0]
            try:
                plan.init_column_means('b', [(0, twice), views_b[1]])
                raise AssertionError('a column chosen twice went through')
            except ValueError:
                pass
        finally:
            for p in (plan, plan_m, plan_o):
                p.close()


def refusals_without_device(lib, ptr):
    """What answers before any HIP call, on the product library without a device (`ptr`: any non-null, 256-byte aligned
    address; never dereferenced)."""
    INV = nat.SKF_E_INVALID
    need = C.c_size_t(7)
    view = (nat.InitView * 1)()
    view[0].rel, view[0].take, view[0].sel = 0, 3, ptr
    assert lib.skf_plan_init_column_means_workspace_bytes(None, 0, 1, view, C.byref(need)) == INV and need.value == 7
    assert b'null' in lib.skf_last_error()
    assert lib.skf_plan_init_column_means(None, 0, 1, view, ptr, 8, ptr, 1 << 20, None) == INV
    assert lib.skf_plan_relation_norms_workspace_bytes(None, 0, C.byref(need)) == INV and need.value == 7
    assert lib.skf_plan_relation_norms(None, 0, ptr, ptr, ptr, 1 << 20, None) == INV


# ---- 4. public API -------------------------------------------------------------------------------------------------------------
def api_graph(kind, sizes=(67, 131, 40), ranks=(5, 7, 5)):
    """kind 'dense' (ratings), 'binary' (0/1), 'sparse' (the ratings as scipy.sparse, unstored = zero), 'masked' (the first
    relation a MaskedArray: Dfmc completes it), 'narrow' (the second relation has 4 columns)."""
    from skfusion_amd.fusion import FusionGraph, Relation, ObjectType
    if kind == 'narrow':
        sizes = (sizes[0], sizes[1], 4)
    types = [ObjectType(n, r) for n, r in zip(TYPES, ranks)]
    host, _ = relations(sizes, 'binary' if kind == 'binary' else 'ratings', 'dense')
    rels = []
    for (i, j), m in host.items():
        data = m
        if kind == 'sparse':
            data = scipy.sparse.csr_matrix(m)
        elif kind == 'masked' and (i, j) == ('a', 'b'):
            data = np.ma.MaskedArray(m, mask=np.random.RandomState(2).rand(*m.shape) < 0.3)
        rels.append(Relation(data, types[TYPES.index(i)], types[TYPES.index(j)], name='%s%s' % (i, j)))
    return FusionGraph(rels)


def fit(cls, graph, seed, max_iter=3, **kw):
    """(fuser, the next draw of the shared RandomState after the fit)"""
    rs = np.random.RandomState(seed)
    fuser = cls(max_iter=max_iter, random_state=rs, **kw).fuse(graph)
    return fuser, rs.randint(1 << 30)


def same_fits(a, b, graph):
    for t in graph.object_types:
        for fa, fb in zip(a.factors_[t], b.factors_[t]):
            assert fa.tobytes() == fb.tobytes(), 'factor of %s differs' % t
    for r in graph.relations:
        for sa, sb in zip(a.backbones_[r], b.backbones_[r]):
            assert sa.tobytes() == sb.tobytes(), 'backbone of %s differs' % r.name


def _no_host_initialiser(monkeypatch):
    from skfusion_amd.fusion.decomposition import dfmf as dfmf_mod, _dfmf as _dfmf_mod

    def boom(*a, **kw):
        raise AssertionError('the host initialiser was reached')
    for mod in (_init, dfmf_mod, _dfmf_mod):
        monkeypatch.setattr(mod, 'initialize', boom)
        monkeypatch.setattr(mod, 'host_view', boom)


def api_case(cls_name, dtype, kind, init_type, monkeypatch, n_run=1, n_jobs=1):
    """init_device=True == init_device=False byte for byte; the device fit never reaches the host initialiser."""
    import skfusion_amd.fusion as F
    cls = getattr(F, cls_name)
    graph = api_graph(kind)
    kw = dict(dtype=dtype, init_type=init_type, n_run=n_run, n_jobs=n_jobs)
    if kind == 'sparse':
        kw['sparse_relations'] = True
    host, draw_h = fit(cls, graph, 4, init_device=False, **kw)
    assert host.init_on_device_ is False
    stay, draw_n = fit(cls, graph, 4, **kw)                 # init_device=None: these sizes stay on the host
    assert stay.init_on_device_ is False and draw_n == draw_h
    same_fits(stay, host, graph)
    with monkeypatch.context() as mp:
        _no_host_initialiser(mp)
        if kind == 'sparse':
            def dense(*a, **k):
                raise AssertionError('a sparse matrix was densified')
            for c in (scipy.sparse.csr_matrix, scipy.sparse.csc_matrix, scipy.sparse.coo_matrix):
                mp.setattr(c, 'toarray', dense)
                mp.setattr(c, 'todense', dense)
        dev, draw_d = fit(cls, graph, 4, init_device=True, **kw)
    assert dev.init_on_device_ is True
    assert draw_d == draw_h, 'the shared RandomState was consumed differently'
    same_fits(dev, host, graph)


def ineligible_case(cls_name, what, dtype='f64'):
    """Fits that initialise on the host whatever init_device says: equal to init_device=False, init_on_device_ False."""
    import skfusion_amd.fusion as F
    cls = getattr(F, cls_name)
    graph = api_graph({'masked': 'masked', 'narrow': 'narrow'}.get(what, 'dense'))
    # (4 columns: take = 0 and the reference's mean of nothing -- NaN factors on either path, which are compared as the
    #  initialiser leaves them and not iterated)
    kw = dict(dtype=dtype, init_type='random' if what == 'random' else 'random_c', max_iter=0 if what == 'narrow' else 3)
    host, draw_h = fit(cls, graph, 6, init_device=False, **kw)
    dev, draw_d = fit(cls, graph, 6, init_device=True, **kw)
    assert host.init_on_device_ is False and dev.init_on_device_ is False and draw_d == draw_h
    if what == 'narrow':
        for t in graph.object_types:
            assert np.array_equal(dev.factors_[t][0], host.factors_[t][0], equal_nan=True)
        return
    same_fits(dev, host, graph)


def device_fill_case(dtype, monkeypatch):
    """device_fill=True with the default init_type: the relations are filled on the device and the host never forms the
    filled matrix."""
    from skfusion_amd.fusion import Dfmf, Relation
    graph = api_graph('dense')
    for r in graph.relations:
        r.data = r.data.copy()
        r.data[3, 2] = np.nan

    def boom(*a, **kw):
        raise AssertionError('a relation was filled on the host')
    with monkeypatch.context() as mp:
        mp.setattr(Relation, 'filled', boom)
        _no_host_initialiser(mp)
        dev, _ = fit(Dfmf, graph, 8, init_device=True, device_fill=True, dtype=dtype)
    assert dev.init_type == 'random_c' and dev.init_on_device_ is True
    for t in graph.object_types:
        assert np.isfinite(dev.factors_[t][0]).all()
    # the host fill and the host initialiser on the same graph agree to the engine's precision
    host, _ = fit(Dfmf, graph, 8, init_device=False, device_fill=False, dtype=dtype)
    tol = {'f64': 1e-9, 'f32': 1e-3}[dtype]
    for t in graph.object_types:
        a, b = dev.factors_[t][0], host.factors_[t][0]
        assert np.linalg.norm(a - b) <= tol * np.linalg.norm(b)
