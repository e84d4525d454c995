"""The column-mean initialisers on the device for relations with MISSING values (csrc/skf_init.h: init_list_means_kernel,
norms_filled_kernel; skf_plan_relation_norms_filled, skf_plan_init_column_means_filled; `init_device` of Dfmf / Dfmc on
``Relation(sp, ..., unstored='unknown')``) against the host initialiser `_init.initialize` / `_init._KnownView` -- shared by
the emulator (a subset) and the GPU tests.

The graph of every plan-level case is the one of init_device_cases.py: types a, b, c, relations (a, b) and (b, c).  (a, b) is
the relation with missing values -- `form` 'known': its known entries over a constant (Dfmc, SKF_REL_KNOWN_CSR), 'rank1':
entries plus rank one (SKF_REL_SPARSE_CSR | SKF_REL_FILL_RANK1) --, (b, c) a dense one, so that type b is touched by a view
over a fill (the transpose of the first relation) and by a dense view: the mixed type.

1. exact data: stored values multiples of 0.5 in [0.5, 5], dyadic fills, so that every sum of the statement is exact:
   byte for byte against `_init.initialize`, pools and random stream included.  The builder itself checks that the host
   norms of such data are exact.  (Not as "the squares of the host norms equal the model's sq": a rounded root squared
   does not give its argument back -- sqrt(2)^2 != 2.  The check is the one the pools hang on: every host norm IS the
   correctly rounded root of the model's exactly summed sq, and the dense sum of squares, added without rounding error by
   math.fsum, is that sq.)
2. real-valued data against a float64 model fed the plan's own lists, under a derived bound (below)
3. line norms, mask-fed == CSR-fed, the mixed type in both view orders, refusals under guard bands, the public API."""
import ctypes as C
import math

import numpy as np
import scipy.sparse

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, KnownEntries
from skfusion_amd.fusion.decomposition import _init

import init_device_cases as IC

TYPES = IC.TYPES
U = IC.U
FILLS = {'known': (2.5,), 'rank1': (2.5, 'mean', 'row_mean', 'col_mean')}


# ---- data ----------------------------------------------------------------------------------------------------------------------
def _pow2_below(n):
    return 1 << (int(n).bit_length() - 1)


def pattern(shape, fill, seed, flip=False):
    """The stored pattern (bool, shape) of the relation with missing values, 5 - 30 % of the cells.
    A number: line 0 EMPTY, line 1 FULL (take - count = 0 for every factor column), every other line at a density of its
    own -- lines: rows, with `flip` columns; 'mean': the same with a power-of-two total; 'row_mean' / 'col_mean': a
    power-of-two count in every line of the averaged side, and on the other side line 0 empty and line 1 full."""
    rs = np.random.RandomState(seed)
    if fill in ('row_mean', 'col_mean'):
        n, m = shape if fill == 'row_mean' else shape[::-1]
        P = np.zeros((n, m), dtype=bool)
        top = int(math.log2(0.3 * m))
        for r in range(n):
            count = 1 << rs.randint(0, top + 1)
            P[r, 1] = True
            P[r, 2 + rs.permutation(m - 2)[:count - 1]] = True
        return P if fill == 'row_mean' else P.T.copy()
    n, m = shape[::-1] if flip else shape
    P = rs.rand(n, m) < (0.05 + 0.25 * rs.rand(n))[:, None]
    P[0], P[1] = False, True
    if fill == 'mean':
        extra = int(P.sum()) - _pow2_below(P.sum())
        r, c = np.nonzero(P[2:])
        drop = rs.permutation(r.size)[:extra]
        P[2 + r[drop], c[drop]] = False
        assert int(P.sum()) == _pow2_below(P.sum())
    return P.T.copy() if flip else P


def sparse_relation(shape, fill, seed, flip=False, real=None, empty=False):
    """`real`: None = exact data; else the engine whose master type the Gaussian values are rounded to first (the reference
    reads the values the plan holds)."""
    rs = np.random.RandomState(seed + 100)
    P = np.zeros(shape, dtype=bool) if empty else pattern(shape, fill, seed, flip)
    V = (np.floor(rs.rand(*shape) * 10.0) + 1.0) * 0.5
    if real:
        V = rs.randn(*shape).astype(nat.NP_DTYPE[nat.DTYPES[real]]).astype(np.float64)
    s = scipy.sparse.csr_matrix((V[P], np.nonzero(P)[1], np.concatenate([[0], np.cumsum(P.sum(axis=1))])), shape=shape)
    s.sort_indices()
    return s


def entries_of(sp, form, fill):
    """The KnownEntries the fit would hand to the plan: Relation.known_entries() / Relation.filled_entries()."""
    from skfusion_amd.fusion import Relation, ObjectType
    rel = Relation(sp, ObjectType('a', 2), ObjectType('b', 2), unstored='unknown', fill_value=fill)
    return rel.known_entries() if form == 'known' else rel.filled_entries()


def relations(sizes, form, fill, seed=3, flip=False, real=None, empty=False):
    """(host dict R_first, rel_list for DevicePlan, variant)"""
    sp = sparse_relation(sizes[:2], fill, seed, flip, real, empty)
    ke = entries_of(sp, form, fill)
    shape = (sizes[1], sizes[2])
    dense = IC.exact_relation(shape, 'ratings', seed + 1)
    if real:
        dense = np.random.RandomState(seed + 1).rand(*shape).astype(nat.NP_DTYPE[nat.DTYPES[real]]).astype(np.float64)
    host = {('a', 'b'): ke, ('b', 'c'): dense}
    rels = [('a', 'b', ke, None), ('b', 'c', dense, None)]
    return host, rels, nat.SKF_DFMC if form == 'known' else nat.SKF_DFMF


def model_sq(ke, transposed):
    """sq of every column of the view as the statement has it, in float64 (exact on exact data)."""
    view = _init._KnownView(ke, transposed)
    n, m = view.shape
    cnt = np.bincount(view.cols, minlength=m)
    if view.a is None:
        return np.bincount(view.cols, weights=view.values ** 2, minlength=m) + (n - cnt) * view.fill ** 2
    stored = np.bincount(view.cols, weights=view.values ** 2, minlength=m)       # (d + a b)^2 = v^2
    return stored + view.b ** 2 * ((view.a ** 2).sum() - np.bincount(view.cols, weights=view.a[view.rows] ** 2, minlength=m))


def host_norms_are_exact(ke):
    """On the CPU, in the builder: every host norm is the correctly rounded root of the model's sq, and that sq is the sum
    of the squares of the dense column without a rounding error."""
    dense = ke.toarray()
    for transposed in (False, True):
        view = _init._KnownView(ke, transposed)
        sq = model_sq(ke, transposed)
        V = dense.T if transposed else dense
        assert all(math.fsum(V[:, k] ** 2) == sq[k] for k in range(V.shape[1]))
        assert np.asarray(view.column_norms()).tobytes() == np.sqrt(sq).tobytes()


def make_plan(sizes, ranks, rels, dtype, variant):
    return IC.make_plan(sizes, ranks, rels, dtype, variant)


# ---- 1. exact data ---------------------------------------------------------------------------------------------------------------
def exact_case(dtype, sizes, ranks, form, fill, init_type, flip=False, empty=False, seed=5):
    host, rels, variant = relations(sizes, form, fill, flip=flip, empty=empty)
    if sizes[0] * sizes[1] <= 1 << 14:
        host_norms_are_exact(host['a', 'b'])
    plan, n_obj, rank = make_plan(sizes, ranks, rels, dtype, variant)
    try:
        got, pools, rs_d = IC.device_init(plan, n_obj, rank, host, init_type, seed)
        want, hpools, rs_h = IC.host_init(n_obj, rank, host, init_type, seed)
        npd = nat.NP_DTYPE[nat.DTYPES[dtype]]
        what = (dtype, form, fill, init_type, flip)
        for t in TYPES:
            up = want[t].astype(npd).astype(np.float64)
            assert got[t].shape == up.shape
            assert got[t].tobytes() == up.tobytes(), 'factor of %s differs from _init.initialize %r' % (t, what)
        if init_type == 'random_c':
            assert sorted(pools) == sorted(hpools)
            for key in hpools:
                assert np.array_equal(pools[key], np.asarray(hpools[key])), 'pool of view %r %r' % (key, what)
        assert rs_d.randint(1 << 30) == rs_h.randint(1 << 30), 'the random stream was consumed differently'
    finally:
        plan.close()


def host_part(view, sel):
    """|mean of the chosen columns| per factor column, as `_column_means_init` forms it for one view."""
    n = view.shape[0]
    part = np.zeros((n, sel.shape[0]))
    for k in range(sel.shape[0]):
        part[:, k] = view.row_means(sel[k]) if isinstance(view, _init._KnownView) else view[:, sel[k]].mean(axis=1)
    return np.abs(part)


def chosen_columns_case(dtype, form, fill, sizes=(67, 131, 40), ranks=(5, 7, 5)):
    """Hand-made selections on the pattern with its empty and its full line: view column 0 is chosen by EVERY factor column,
    view column 1 by NONE, in both orientations of the relation with missing values; then the mixed type b in BOTH view
    orders.  Byte for byte against the host's statement."""
    host, rels, variant = relations(sizes, form, fill)
    ke = host['a', 'b']
    plan, n_obj, rank = make_plan(sizes, ranks, rels, dtype, variant)
    npd = nat.NP_DTYPE[nat.DTYPES[dtype]]
    rs = np.random.RandomState(11)

    def selection(m, c):
        take = int(.2 * m)
        return np.stack([np.concatenate([[0], 2 + rs.permutation(m - 2)[:take - 1]]) for _ in range(c)])
    try:
        sel_a = selection(sizes[1], ranks[0])
        plan.init_column_means('a', [(0, sel_a)])
        want = 1e-5 + host_part(_init._KnownView(ke, False), sel_a)
        assert plan.get_factor('a').tobytes() == want.astype(npd).astype(np.float64).tobytes()
        sel_t, sel_d = selection(sizes[0], ranks[1]), selection(sizes[2], ranks[1])
        parts = {0: host_part(_init._KnownView(ke, True), sel_t), 1: host_part(host['b', 'c'], sel_d)}
        for order in ((0, 1), (1, 0)):
            plan.init_column_means('b', [(q, (sel_t, sel_d)[q]) for q in order])
            want = np.full((sizes[1], ranks[1]), 1e-5)
            for q in order:
                want += parts[q]
            assert plan.get_factor('b').tobytes() == want.astype(npd).astype(np.float64).tobytes(), order
    finally:
        plan.close()


# ---- line norms ----------------------------------------------------------------------------------------------------------------
def norms_case(dtype, sizes, form, fill, flip=False):
    host, rels, variant = relations(sizes, form, fill, flip=flip)
    ke = host['a', 'b']
    plan, _, _ = make_plan(sizes, (5, 7, 5), rels, dtype, variant)
    try:
        rs, cs = plan.relation_norms(0)
        assert cs.tobytes() == model_sq(ke, False).tobytes() and rs.tobytes() == model_sq(ke, True).tobytes(), (dtype, form, fill)
        again = plan.relation_norms(0)
        assert again[0].tobytes() == rs.tobytes() and again[1].tobytes() == cs.tobytes()
        dense = host['b', 'c'] ** 2                         # (the dense relation beside it: the unchanged path)
        rs, cs = plan.relation_norms(1)
        assert rs.tobytes() == dense.sum(axis=1).tobytes() and cs.tobytes() == dense.sum(axis=0).tobytes()
    finally:
        plan.close()


# ---- the forms the older entry points take: same launches, same bits ---------------------------------------------------------------
def launches(rt):
    count = C.c_int64()
    rt.call('skf_launch_count', C.byref(count))
    return count.value


def unchanged_route_case(dtype, form, sizes=(67, 131, 40), ranks=(5, 7, 5)):
    """A plan without a relation over a fill (`form` 'dense' | 'csr', init_device_cases.relations): the `_filled` entry points
    give the bytes of the older ones with the same number of launches, and the plan object keeps calling the older ones."""
    host, rels = IC.relations(sizes, 'ratings', form)
    plan, n_obj, rank = IC.make_plan(sizes, ranks, rels, dtype)
    rs = np.random.RandomState(17)
    views = [(0, np.stack([rs.permutation(67)[:13] for _ in range(7)])), (1, np.stack([rs.permutation(40)[:8] for _ in range(7)]))]
    try:
        assert not plan.rel_over_fill
        old, new = IC.Raw(plan, 'b', views), Raw(plan, 'b', views, None)
        assert old.need() == new.need()
        old.scratch(old.need())
        new.scratch(new.need())
        n0 = launches(plan.rt)
        assert old.call() == 0
        n1 = launches(plan.rt)
        assert new.call() == 0
        n2 = launches(plan.rt)
        assert n1 - n0 == n2 - n1 > 0 and old.result().tobytes() == new.result().tobytes()
        mem = plan.rt.mem
        sq = [mem.empty(131 * 8) for _ in range(4)]
        need = C.c_size_t()
        plan.rt.call('skf_plan_relation_norms_filled_workspace_bytes', plan.handle, 1, C.byref(need))
        ws = mem.empty(max(need.value, 1))
        n0 = launches(plan.rt)
        plan.rt.call('skf_plan_relation_norms', plan.handle, 1, sq[0].ptr, sq[1].ptr, ws.ptr, need.value, plan.stream)
        n1 = launches(plan.rt)
        plan.rt.call('skf_plan_relation_norms_filled', plan.handle, 1, 0.0, sq[2].ptr, sq[3].ptr, ws.ptr, need.value, plan.stream)
        n2 = launches(plan.rt)
        mem.synchronize()
        assert n1 - n0 == n2 - n1 > 0
        assert mem.to_host(sq[0], (131,), np.float64).tobytes() == mem.to_host(sq[2], (131,), np.float64).tobytes()
        assert mem.to_host(sq[1], (40,), np.float64).tobytes() == mem.to_host(sq[3], (40,), np.float64).tobytes()
    finally:
        plan.close()


# ---- mask-fed equals CSR-fed ---------------------------------------------------------------------------------------------------
def mask_fed_case(dtype, sizes=(67, 131, 40), ranks=(5, 7, 5), fill=2.5):
    """A SKF_DFMC plan whose masked dense relation is kept as lists (known_bound) gives, through the new entry points, the
    bytes of the SKF_REL_KNOWN_CSR plan of the same data."""
    host, rels, variant = relations(sizes, 'known', fill)
    ke = host['a', 'b']
    known = np.zeros(ke.shape, dtype=bool)
    rows, cols = ke.rows_cols()
    known[rows, cols] = True
    fed = [('a', 'b', ke.toarray(), ~known), rels[1]]
    plan_c, n_obj, rank = make_plan(sizes, ranks, rels, dtype, variant)
    plan_m = DevicePlan(TYPES, n_obj, rank, fed, [], variant, dtype=dtype, sparse_known=None)
    rs = np.random.RandomState(13)
    try:
        lists_m, lists_c = plan_m.relation_lists(0), plan_c.relation_lists(0)         # (the mask form IS kept as lists)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(lists_m, lists_c))
        nm, nc = plan_m.relation_norms(0, fill=fill), plan_c.relation_norms(0)
        assert nm[0].tobytes() == nc[0].tobytes() and nm[1].tobytes() == nc[1].tobytes()
        sel_a = np.stack([rs.permutation(sizes[1])[:26] for _ in range(ranks[0])])
        sel_t = np.stack([rs.permutation(sizes[0])[:13] for _ in range(ranks[1])])
        sel_d = np.stack([rs.permutation(sizes[2])[:8] for _ in range(ranks[1])])
        plan_m.init_column_means('a', [(0, sel_a, fill)])
        plan_c.init_column_means('a', [(0, sel_a)])
        plan_m.init_column_means('b', [(0, sel_t, fill), (1, sel_d)])
        plan_c.init_column_means('b', [(0, sel_t), (1, sel_d)])
        for t in 'ab':
            assert plan_m.get_factor(t).tobytes() == plan_c.get_factor(t).tobytes(), t
    finally:
        plan_m.close()
        plan_c.close()


# ---- 2. real-valued data -------------------------------------------------------------------------------------------------------
# The model: the statement of skf_init.h in float64 on the plan's OWN list values (skf_get_relation_lists; a / b as uploaded,
# i.e. cast to the master type), every sum sequential in list order (np.bincount adds its weights in input order), B_k
# sequential in the order of sel (np.cumsum), the epilogue a product rounded, then a sum rounded (NumPy fuses nothing; the
# kernels are compiled with contraction off).  The device runs the same operations in the same order, so it may differ from
# the model by the final rounding to the master type alone; the host initialiser differs from it by
#   * the values it reads: v where the lists hold d = fl(v - a b) -- one rounding of the master type per stored entry, u_m |d|
#   * known + a (B - b_stored) where the model has sum d + a B: sums of up to take + 1 terms each, take u64 of their moduli
#   * B pairwise (NumPy) against sequential: (take - 1) u64 sum |b|
# Per view and element, with S = sum over the stored chosen of (|v| + |a b|) + |a| sum over the chosen of |b| (known form:
# S = sum |v| + (take - count) |f|):
#   bound = FACTOR * ((take + 3) u64 + u_lists) S / take, summed over the views, + 2 u_m |G|        (u_lists = u_m for rank
# one in an f32 engine, where a, b and d are rounded to f32; 0 otherwise: the stored values are rounded to the master type
# before either side reads them)
# and for the dense view beside it the term of init_device_cases.py, 2 take u mean|v| with u = u64 for the host and u_m for
# the device, whose product runs in the master type.
# The host initialiser is held to this bound as derived (factor 1), the device to FACTOR_DEVICE times it: at most 10 x the
# largest share of the bound seen on the hardware (profiles/init_known.txt), and never above the derived bound itself.
FACTOR_DEVICE = 1.0


def list_model(plan, host, n_obj, rank, views_of, dtype):
    """(G, B, D) per type in float64 from the plan's lists: the model, the bound of the views over a fill and the
    coefficient of u of the dense views."""
    ke = host['a', 'b']
    npd = nat.NP_DTYPE[nat.DTYPES[dtype]]
    lists = {False: plan.relation_lists(0), True: plan.relation_lists(0, by_col=True)}
    rank1 = ke.row_fill is not None
    fa = ke.row_fill.astype(npd).astype(np.float64) if rank1 else None
    fb = ke.col_fill.astype(npd).astype(np.float64) if rank1 else None
    u_lists = U[dtype] if rank1 and dtype != 'f64' else 0.0
    G, B, D = {}, {}, {}
    for t, views in views_of.items():
        n, c = n_obj[t], rank[t]
        acc, bnd, dns = np.full((n, c), 1e-5), np.zeros((n, c)), np.zeros((n, c))
        for rel, transposed, sel in views:
            take = sel.shape[1]
            if rel == 1:
                V = host['b', 'c'].T if transposed else host['b', 'c']
                for k in range(c):
                    acc[:, k] += np.abs(V[:, sel[k]].mean(axis=1))
                    dns[:, k] += 2.0 * take * np.abs(V[:, sel[k]]).sum(axis=1) / take
                continue
            ptr, idx, val = lists[transposed]
            val = val.astype(np.float64)
            line = np.repeat(np.arange(n), np.diff(ptr))
            own, other = (fb, fa) if transposed else (fa, fb)
            m = ke.shape[0] if transposed else ke.shape[1]
            for k in range(c):
                flag = np.zeros(m, dtype=bool)
                flag[sel[k]] = True
                hit = flag[idx]
                s = np.bincount(line[hit], weights=val[hit], minlength=n)
                cnt = np.bincount(line[hit], minlength=n)
                if rank1:
                    Bk = np.cumsum(other[sel[k]])[-1]
                    beneath = own * Bk
                    ab = np.abs(own[line[hit]] * other[idx[hit]])
                    S = (np.bincount(line[hit], weights=2.0 * ab + np.abs(val[hit]), minlength=n) +
                         np.abs(own) * np.abs(other[sel[k]]).sum())
                else:
                    beneath = (take - cnt).astype(np.float64) * ke.fill
                    S = np.bincount(line[hit], weights=np.abs(val[hit]), minlength=n) + (take - cnt) * abs(ke.fill)
                acc[:, k] += np.abs((s + beneath) / take)
                bnd[:, k] += ((take + 3) * U['f64'] + u_lists) * S / take
        G[t], B[t], D[t] = acc, bnd, dns
    return G, B, D


def real_case(dtype, sizes, ranks, form, fill, init_type='random_vcol', seed=9, check_host=True):
    """Gaussian values, arbitrary counts: the device against the list model under the bound; the host initialiser too (it is
    the CPU check that the bound holds: it needs a plan for the lists only)."""
    host, rels, variant = relations(sizes, form, fill, real=dtype)
    plan, n_obj, rank = make_plan(sizes, ranks, rels, dtype, variant)
    npd = nat.NP_DTYPE[nat.DTYPES[dtype]]
    try:
        rs = np.random.RandomState(seed)
        shapes = {k: v.shape for k, v in host.items()}
        pos = _init.draw_positions(TYPES, rank, shapes, init_type, rs)
        assert init_type == 'random_vcol'       # (`random_c` on real data: a flipped near-tie of two norms is another valid draw)
        views_of = {t: [(0 if pair == ('a', 'b') else 1, tr, p) for (pair, tr), p in pos[t]] for t in TYPES}
        got, _, _ = IC.device_init(plan, n_obj, rank, host, init_type, seed)
        G, B, D = list_model(plan, host, n_obj, rank, views_of, dtype)
        want, _, _ = IC.host_init(n_obj, rank, host, init_type, seed)
        worst_d = worst_h = 0.0
        for t in TYPES:
            if check_host:
                bound = B[t] + U['f64'] * D[t] + 2 * U['f64'] * np.abs(G[t])
                worst_h = max(worst_h, float((np.abs(want[t] - G[t]) / bound).max()))
            bound = FACTOR_DEVICE * (B[t] + U[dtype] * D[t] + 2 * U[dtype] * np.abs(G[t]))
            worst_d = max(worst_d, float((np.abs(got[t] - G[t]) / bound).max()))
        # (type a has the view over a fill alone: the same operations in the same order as the model, then one rounding)
        exact = got['a'].tobytes() == G['a'].astype(npd).astype(np.float64).tobytes()
        print('init_known real %s %s %r %r %r: device / its bound %.3g (type a equals the rounded model: %s), host / bound %.3g'
              % (dtype, form, fill, sizes, ranks, worst_d, exact, worst_h))
        assert worst_h <= 1.0, 'the host initialiser leaves the bound: %.3g' % worst_h
        assert worst_d <= 1.0, 'the device leaves the bound: %.3g' % worst_d
    finally:
        plan.close()


# ---- 3. refusals and guards ----------------------------------------------------------------------------------------------------
class Raw(IC.Raw):
    """init_device_cases.Raw through the `_filled` entry points, with the fills of the views."""

    def __init__(self, plan, t, views, fills, ld=None):
        IC.Raw.__init__(self, plan, t, views, ld)
        self.fills = (C.c_double * len(views))(*fills) if fills is not None else None

    def need(self):
        need = C.c_size_t()
        self.rt.call('skf_plan_init_column_means_filled_workspace_bytes', self.plan.handle, self.k, self.nv, self.desc, C.byref(need))
        return need.value

    def call(self, ws_bytes=None, ws=True, g0=True, ld=None, shift=0):
        rc = self.rt.lib.skf_plan_init_column_means_filled(
            self.plan.handle, self.k, self.nv, self.desc, self.fills, self.g0.ptr if g0 else None, self.ld if ld is None else ld,
            (self.ws.ptr + shift) if ws else None, len(self.ws_pat) if ws_bytes is None else ws_bytes, self.plan.stream)
        self.rt.mem.synchronize()
        return rc


def refusals_case(dtype='f32'):
    """Every refusal of the `_filled` entry points before any write, the scratch as it was; ld > c keeps the padding."""
    from guarded import guarded
    from skfusion_amd.fusion.decomposition._dfmf import owned_plan
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    sizes, ranks = (67, 131, 40), (5, 7, 5)
    with guarded():
        host, rels, variant = relations(sizes, 'known', 2.5)
        _, rels1, variant1 = relations(sizes, 'rank1', 'row_mean')
        plan, n_obj, rank = make_plan(sizes, ranks, rels, dtype, variant)
        plan1, _, _ = make_plan(sizes, ranks, rels1, dtype, variant1)
        dense = host["a", "b"].toarray()
        masked = [('a', 'b', dense, dense == 2.5), rels[1]]
        plan_m = DevicePlan(TYPES, n_obj, rank, masked, [], nat.SKF_DFMC, dtype=dtype, sparse_known=False)       # kept DENSE
        plan_o = owned_plan(nat.SKF_DFMC, [('a', 'b', host['a', 'b'], None), rels[1]], [], TYPES, n_obj, rank, dtype, None, 0, 1)
        try:
            rs = np.random.RandomState(1)
            good = lambda m, c, take: np.stack([rs.permutation(m)[:take] for _ in range(c)])
            views_b = [(0, good(67, 7, 13)), (1, good(40, 7, 8))]
            fills_b = [2.5, 0.0]
            for p in (plan, plan1):
                # an index out of range, in either view: found on the device before anything is written
                for which, bad in ((1, 40), (1, -1), (0, 67)):
                    v = [(0, views_b[0][1].copy()), (1, views_b[1][1].copy())]
                    v[which][1][6, 7] = bad
                    raw = Raw(p, 'b', v, fills_b)
                    raw.scratch(raw.need())
                    assert raw.call() == INV and b'outside its view' in raw.rt.lib.skf_last_error() and raw.untouched(), bad
                # take == 0 and take > m
                for take in (0, 68):
                    raw = Raw(p, 'b', [(0, np.zeros((7, take), dtype=np.int32)), views_b[1]], fills_b)
                    raw.scratch(1 << 16)
                    assert raw.call() == INV and raw.untouched(), take
                # a relation that does not touch the type; a relation index out of range
                for rel in (1, 2, -1):
                    raw = Raw(p, 'a', [(rel, good(131, 5, 26))], [2.5])
                    raw.scratch(1 << 16)
                    assert raw.call() == INV and raw.untouched(), rel
                # a short, a missing and a misaligned scratch; ld < c; a null output
                raw = Raw(p, 'b', views_b, fills_b)
                nb = raw.need()
                raw.scratch(nb + 256)
                assert raw.call(ws_bytes=nb - 1) == WS and raw.call(ws=False) == WS and raw.call(ws_bytes=nb, shift=8) == WS
                assert raw.call(ws_bytes=nb, ld=6) == INV and raw.call(ws_bytes=nb, g0=False) == INV
                assert raw.untouched()
                # ld > c: the padding of every row stays; the values are those of the packed call
                packed = Raw(p, 'b', views_b, fills_b)
                packed.scratch(nb)
                assert packed.call() == 0
                wide = Raw(p, 'b', views_b, fills_b, ld=10)
                wide.scratch(nb)
                assert wide.call() == 0
                got = wide.result()
                assert got[:, :7].tobytes() == packed.result().tobytes()
                assert got[:, 7:].tobytes() == wide.g_pat.view(p.np_dtype).reshape(131, 10)[:, 7:].tobytes()
            # a fill that is not finite, missing fills (known-entry views only: the rank-one plan needs none)
            for f in (float('nan'), float('inf')):
                raw = Raw(plan, 'b', views_b, [f, 0.0])
                raw.scratch(raw.need())
                assert raw.call() == INV and b'not finite' in raw.rt.lib.skf_last_error() and raw.untouched()
                assert raw.rt.lib.skf_plan_relation_norms_filled(plan.handle, 0, f, raw.g0.ptr, None, raw.ws.ptr, 1 << 16, plan.stream) == INV
                assert raw.untouched()
            raw = Raw(plan, 'b', views_b, None)
            raw.scratch(raw.need())
            assert raw.call() == INV and raw.untouched()
            raw = Raw(plan1, 'b', views_b, None)
            raw.scratch(raw.need())
            assert raw.call() == 0
            # a masked relation the plan keeps dense, and a plan with owned rows: both operators refuse
            for p in (plan_m, plan_o):
                raw = Raw(p, 'a', [(0, good(131, 5, 26))], [2.5])
                raw.scratch(1 << 16)
                assert raw.call() == INV and raw.untouched()
                need = C.c_size_t()
                assert raw.rt.lib.skf_plan_init_column_means_filled_workspace_bytes(p.handle, 0, 1, raw.desc, C.byref(need)) == INV
                assert raw.rt.lib.skf_plan_relation_norms_filled(p.handle, 0, 2.5, raw.g0.ptr, None, raw.ws.ptr, 1 << 16, p.stream) == INV
                assert raw.untouched()
            # (the unmasked relation of the dense-masked plan is covered, through the unchanged route)
            raw = Raw(plan_m, 'c', [(1, good(131, 5, 26))], None)
            raw.scratch(raw.need())
            assert raw.call() == 0
            # the old entry points still refuse the two forms
            old = IC.Raw(plan, 'a', [(0, good(131, 5, 26))])
            old.scratch(1 << 16)
            assert old.call() == INV and old.untouched()
            # the binding refuses a column chosen twice for one factor column
            twice = views_b[0][1].copy()
            twice[3, 5] = twice[3, 0]
            try:
                plan.init_column_means('b', [(0, twice), views_b[1]])
                raise AssertionError('a column chosen twice went through')
            except ValueError:
                pass
        finally:
            for p in (plan, plan1, plan_m, plan_o):
                p.close()


def refusals_without_device(lib, ptr):
    """What answers before any HIP call, on the product library without a device."""
    INV = nat.SKF_E_INVALID
    need = C.c_size_t(7)
    view = (nat.InitView * 1)()
    view[0].rel, view[0].take, view[0].sel = 0, 3, ptr
    fills = (C.c_double * 1)(2.5)
    assert lib.skf_plan_init_column_means_filled_workspace_bytes(None, 0, 1, view, C.byref(need)) == INV and need.value == 7
    assert b'null' in lib.skf_last_error()
    assert lib.skf_plan_init_column_means_filled(None, 0, 1, view, fills, ptr, 8, ptr, 1 << 20, None) == INV
    assert lib.skf_plan_relation_norms_filled_workspace_bytes(None, 0, C.byref(need)) == INV and need.value == 7
    assert lib.skf_plan_relation_norms_filled(None, 0, 2.5, ptr, ptr, ptr, 1 << 20, None) == INV


# ---- 4. public API -------------------------------------------------------------------------------------------------------------
def api_graph(fill, sizes=(67, 131, 40), ranks=(5, 7, 5)):
    from skfusion_amd.fusion import FusionGraph, Relation, ObjectType
    types = [ObjectType(n, r) for n, r in zip(TYPES, ranks)]
    sp = sparse_relation(sizes[:2], fill, 3)
    dense = IC.exact_relation((sizes[1], sizes[2]), 'ratings', 4)
    return FusionGraph([Relation(sp, types[0], types[1], name='ab', unstored='unknown', fill_value=fill),
                        Relation(dense, types[1], types[2], name='bc')])


def api_case(cls_name, dtype, fill, init_type, monkeypatch, n_run=1, n_jobs=1):
    """init_device=True == init_device=False byte for byte after 3 iterations; the device fit reaches neither the host
    initialiser nor a dense form of the sparse relation; init_device=None stays on the host at these sizes."""
    import skfusion_amd.fusion as F
    cls = getattr(F, cls_name)
    graph = api_graph(fill)
    kw = dict(dtype=dtype, init_type=init_type, n_run=n_run, n_jobs=n_jobs, sparse_relations=True)
    host, draw_h = IC.fit(cls, graph, 4, init_device=False, **kw)
    assert host.init_on_device_ is False
    stay, draw_n = IC.fit(cls, graph, 4, **kw)
    assert stay.init_on_device_ is False and draw_n == draw_h
    IC.same_fits(stay, host, graph)
    with monkeypatch.context() as mp:
        IC._no_host_initialiser(mp)

        def dense(*a, **k):
            raise AssertionError('a sparse matrix was densified')
        for c in (scipy.sparse.csr_matrix, scipy.sparse.csc_matrix, scipy.sparse.coo_matrix):
            mp.setattr(c, 'toarray', dense)
            mp.setattr(c, 'todense', dense)
        dev, draw_d = IC.fit(cls, graph, 4, init_device=True, **kw)
    assert dev.init_on_device_ is True
    assert draw_d == draw_h, 'the shared RandomState was consumed differently'
    IC.same_fits(dev, host, graph)
