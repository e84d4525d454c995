"""Fold-ins through sparse relations given as their stored entries, compressed along the target's side (SKF_REL_FOLD_CSR,
fold_lists_kernel in csrc/skf_known.h, fold_prepare / fold_err_pass in csrc/skf_stages.inc) -- the SAME cases on the host
emulator (small) and on the GPU.

  1. skf_fold_lists bit for bit (fold_lists_case): stored values are multiples of 1/8 in (-8, 8) and T holds multiples of
     1/64 with |.| <= 4, so every product is exact in f32 and an fma has the bits of a multiply and an add; the host model
     is the loop of the header comment -- x = fma(v[k], T[idx[k]][q], x) in list order, then Ec += max(x, 0),
     Dc += max(-x, 0) -- in the engine's type.  np.array_equal, padding behind column c untouched.
  2. whole fold-ins (whole_case): the f64 engine against oracle.dfmf_oracle.transform on the dense matrices within 1e-9
     (the project's standing fold-in bound); f32 / bf16: the dense-fed plan of the same data is the
     yardstick -- its deviation ||G_dense - G_host64|| / ||G_host64|| from the f64 host result, and the list-fed plan may
     deviate at most 2 x that from the same host result (the same number of terms summed in another order).
  3. skf_relation_sqerr on both sides: the first-order bound sparse_dfmf_cases.pass_case derives for the fit's error pass
     (same K_SAFE), and the identity itself against the dense f64 sum to 1e-9.
  4. flags and lists: every SKF_E_INVALID of the header comment."""
import ctypes as C

import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, KnownEntries
from helpers import plan_create_status, relerr, within
import known_cases as K
from dense_cases import constraint


# ---- 1. the stand-alone operator ---------------------------------------------------------------------------------------
def lists_of(pat, values):
    """Row-major lists (indptr, indices, values) of the entries `pat` marks."""
    rows, cols = np.nonzero(pat)
    indptr = np.zeros(pat.shape[0] + 1, dtype=np.int64)
    np.cumsum(pat.sum(axis=1), out=indptr[1:])
    return indptr, cols.astype(np.int32), values[rows, cols]


def host_fold(indptr, indices, values, T, Ec, Dc, c, dtype):
    """The loop of include/skfusion_hip.h (skf_fold_lists) in the engine's type.  Products are exact in that type for the
    test's values, so multiply-then-add rounds once, as the fma does."""
    Ec, Dc = Ec.copy(), Dc.copy()
    for o in range(len(indptr) - 1):
        x = np.zeros(c, dtype=dtype)
        for k in range(int(indptr[o]), int(indptr[o + 1])):
            x = (values[k] * T[indices[k], :c] + x).astype(dtype)
        Ec[o, :c] = Ec[o, :c] + np.maximum(x, dtype(0))
        Dc[o, :c] = Dc[o, :c] + np.maximum(-x, dtype(0))
    return Ec, Dc


def fold_lists_case(n_out, n_partner, c, pattern, dtype, seed=0):
    rt = nat.get_runtime()
    T_ = np.float64 if dtype == 'f64' else np.float32
    rs = np.random.RandomState(seed + c)
    pat = K.edge_mask(n_out, n_partner, pattern, seed)
    vals = (rs.randint(-63, 64, size=pat.shape) / 8.0).astype(T_)
    indptr, indices, values = lists_of(pat, vals)
    ldt, lde, ldd = c + 3, c + 5, c + 2
    Tm = (rs.randint(-256, 257, size=(n_partner, ldt)) / 64.0).astype(T_)
    # accumulators pre-filled with low-bit values (the additions round) and a sentinel behind column c
    Ec = (rs.randint(1, 2 ** 20, size=(n_out, lde)) / float(2 ** 22)).astype(T_)
    Dc = (rs.randint(1, 2 ** 20, size=(n_out, ldd)) / float(2 ** 22)).astype(T_)
    Ec[:, c:] = -77.0
    Dc[:, c:] = -55.0
    keep = lambda a: rt.mem.from_host(a if a.size else np.zeros(1, dtype=a.dtype))
    bp, bi, bv, bt, be, bd = keep(indptr), keep(indices), keep(values), keep(Tm), keep(Ec), keep(Dc)
    rt.call('skf_fold_lists', nat.DTYPES[dtype], bp.ptr, bi.ptr, bv.ptr, n_out, bt.ptr, ldt, c, be.ptr, lde, bd.ptr, ldd,
            rt.mem.stream)
    rt.mem.synchronize()
    gE, gD = rt.mem.to_host(be, Ec.shape, T_), rt.mem.to_host(bd, Dc.shape, T_)
    hE, hD = host_fold(indptr, indices, values, Tm, Ec, Dc, c, T_)
    what = 'skf_fold_lists %s %s n_out %d c %d' % (dtype, pattern, n_out, c)
    assert (hE[:, :c] != Ec[:, :c]).any() and (hD[:, :c] != Dc[:, :c]).any(), what + ': both halves of the split must be hit'
    assert np.array_equal(gE[:, :c], hE[:, :c]), '%s: Ec differs from the host loop (max %.3e)' % (what, np.max(np.abs(gE - hE)))
    assert np.array_equal(gD[:, :c], hD[:, :c]), '%s: Dc differs from the host loop (max %.3e)' % (what, np.max(np.abs(gD - hD)))
    assert np.array_equal(gE[:, c:], Ec[:, c:]) and np.array_equal(gD[:, c:], Dc[:, c:]), what + ': memory past column c changed'


def fold_lists_refusals():
    """SKF_E_INVALID of the operator: a dtype that is not f64 / f32, a null pointer, widths 0 and 1025, a short ld."""
    rt = nat.get_runtime()
    b = rt.mem.empty(4096)
    call = lambda dt, p, c, ld: rt.lib.skf_fold_lists(dt, p, b.ptr, b.ptr, 0, b.ptr, ld, c, b.ptr, ld, b.ptr, ld, rt.mem.stream)
    assert call(nat.SKF_F32, b.ptr, 4, 4) == 0                  # (no output object: nothing is read or launched)
    assert call(nat.SKF_BF16, b.ptr, 4, 4) == nat.SKF_E_INVALID
    assert call(nat.SKF_F32, None, 4, 4) == nat.SKF_E_INVALID
    assert call(nat.SKF_F32, b.ptr, 0, 4) == nat.SKF_E_INVALID
    assert call(nat.SKF_F32, b.ptr, 1025, 1025) == nat.SKF_E_INVALID
    assert call(nat.SKF_F32, b.ptr, 8, 7) == nat.SKF_E_INVALID


# ---- 2. / 3. whole fold-ins --------------------------------------------------------------------------------------------
def signed_eighths(rs, shape):
    """Multiples of 1/8 in (-8, 8), both signs (exact in bf16: the dense bf16 copy of the yardstick holds them unrounded)."""
    return rs.randint(-63, 64, size=shape) / 8.0


def entries_along(R, pat, by_col):
    """KnownEntries(unstored='zero') of the entries `pat` marks, compressed along the rows or (by_col) the columns."""
    if by_col:
        p, i, v = lists_of(pat.T, np.ascontiguousarray(R.T))
    else:
        p, i, v = lists_of(pat, R)
    return KnownEntries(p, i, v, R.shape, unstored='zero', by_col=by_col)


def fold_graph(n, seed, zero_first=False):
    """t x a (edge patterns; an all-zero relation with zero_first), b x t (heavy-tailed), a second t x a, all sparse, and a
    dense t x b; target object 7 holds no entry in any of them.  Returns [(i, j, R, pattern or None)] in dict order."""
    rs = np.random.RandomState(seed)
    nt, na, nb = n['t'], n['a'], n['b']
    pats = [K.edge_mask(nt, na, 'edges', seed, bg=0.05), rs.rand(nt, na) < 0.04, K.edge_mask(nb, nt, 'heavy', seed + 1)]
    if zero_first:
        pats[0][:] = False
    pats[0][7, :] = pats[1][7, :] = False
    pats[2][:, 7] = False
    dense = rs.rand(nt, nb) * 2.0 - 0.6
    dense[7, :] = 0.0
    rels = [('t', 'a', np.where(pats[0], signed_eighths(rs, (nt, na)), 0.0), pats[0]),
            ('t', 'a', np.where(pats[1], signed_eighths(rs, (nt, na)), 0.0), pats[1]),
            ('b', 't', np.where(pats[2], signed_eighths(rs, (nb, nt)), 0.0), pats[2]),
            ('t', 'b', dense, None)]
    return rels, rs


def make_plan(dtype, n, ranks, rels, theta, Gp, S, G0, lists):
    rl = [(i, j, entries_along(R, pat, by_col=(j == 't')) if (lists and pat is not None) else R, None) for i, j, R, pat in rels]
    plan = DevicePlan(['t', 'a', 'b'], n, ranks, rl, [('t', theta)] if theta is not None else [], nat.SKF_TRANSFORM,
                      dtype=dtype, target='t')
    for o in ('a', 'b'):
        plan.set_factor(o, Gp[o])
    plan.set_factor('t', G0)
    for k, s in enumerate(S):
        plan.set_backbone(k, s)
    return plan


def oracle_fold(rels, theta, ranks, Gp, S, G0, iters):
    from oracle import dfmf_oracle as orc
    R, Sd = {}, {}
    for (i, j, M, _), s in zip(rels, S):
        R.setdefault((i, j), []).append(M)
        Sd.setdefault((i, j), []).append(np.asarray(s, dtype=np.float64))
    G = {('a', 'a'): Gp['a'], ('b', 'b'): Gp['b']}
    return orc.transform(R, {('t', 't'): [theta]} if theta is not None else {}, 't', ranks, G, Sd, max_iter=iters, G0=G0)


def sqerr_ratio(dtype, R_tp, pat_tp, Gt, Seff, Gp, got, n_t, n_p, c_t, c_p):
    """|device - host| / (K_SAFE bound) of skf_relation_sqerr, target x partner orientation (R_tp, pattern pat_tp),
    H = G_t Seff (c_t x c_p): the bound of sparse_dfmf_cases.pass_case for the fit's error pass."""
    et = 'f32' if dtype == 'bf16' else dtype                   # (the pass gathers the f32 masters in the bf16 engine)
    u = K.U_ACC[et]
    Hr, dH = K.gathered_T(Gt, Seff.T, et)                       # H = G_t Seff as the pass gathers it
    Gr = K.store_round(Gp, et)
    x = Hr @ Gr.T
    dx = (c_p + 2) * u * (np.abs(Hr) @ np.abs(Gr).T) + dH @ np.abs(Gr).T
    Kf = pat_tp.astype(np.float64)
    X = Gt @ Seff @ Gp.T
    host = np.sum(X * X) + np.sum(Kf * ((R_tp - x) ** 2 - x ** 2))
    bound = np.sum(Kf * (2 * (np.abs(R_tp - x) + np.abs(x)) * dx + 4 * u * ((R_tp - x) ** 2 + x ** 2)))
    bound += (n_t + n_p + 2 * (c_t + c_p)) * 2.0 ** -53 * np.sum((np.abs(Gt) @ np.abs(Seff) @ np.abs(Gp).T) ** 2)
    dense = np.sum((R_tp - X) ** 2)                             # (the formula itself: the dense statement in f64)
    assert abs(np.sum(X * X) + np.sum(Kf * ((R_tp - X) ** 2 - X ** 2)) - dense) <= 1e-9 * dense
    return abs(got - host) / (K.K_SAFE * bound)


def whole_case(dtype, ranks, with_theta, what, n=None, iters=5, seed=0):
    """Five iterations of the list-fed plan (fused iteration; with a constraint on the target: the generic one) against the
    f64 host, iterate(k) against k x iterate(1), relation_sqerr of every list-fed relation, re-preparation after
    skf_set_backbone and after skf_set_factor of a partner.  Returns the measured deviations."""
    n = n or {'t': 131, 'a': 197, 'b': 90}
    rels, rs = fold_graph(n, seed)
    f32 = (lambda a: K.store_round(a, 'f32')) if dtype != 'f64' else (lambda a: a)
    Gp = {o: f32(rs.rand(n[o], ranks[o]) + 0.1) for o in ('a', 'b')}
    S = [f32(rs.rand(ranks[i], ranks[j]) * 2.0 - 0.6) for i, j, _, _ in rels]
    G0 = f32(rs.rand(n['t'], ranks['t']) + 0.1)
    S2 = list(S)
    S2[0] = f32(rs.rand(*S[0].shape) * 2.0 - 1.0)
    Ga2 = f32(rs.rand(n['a'], ranks['a']) + 0.2)
    theta = constraint('csr', n['t'], rs) if with_theta else None
    out = {}

    def run(lists):
        plan = make_plan(dtype, n, ranks, rels, theta, Gp, S, G0, lists)
        try:
            assert plan.batchable() == (theta is None)
            G = [plan.get_factor('t')]
            for _ in range(iters):
                plan.iterate(1)
                G.append(plan.get_factor('t'))
            sq = [plan.relation_sqerr(k) for k in range(len(rels))]
            plan.set_factor('t', G0)
            plan.iterate(iters)
            np.testing.assert_array_equal(plan.get_factor('t'), G[iters], err_msg='%s: iterate(%d) vs %d x iterate(1)' % (what, iters, iters))
            plan.set_backbone(0, S2[0])
            plan.iterate(1)
            Gb = plan.get_factor('t')
            plan.set_factor('a', Ga2)
            plan.iterate(1)
            Gc = plan.get_factor('t')
            if lists:
                with pytest.raises(nat.SkfNativeError) as exc:
                    plan.get_contraction(0, 0)
                assert exc.value.code == nat.SKF_E_INVALID
            return G, sq, Gb, Gc, plan.workspace_bytes
        finally:
            plan.close()

    G, sq, Gb, Gc, ws = run(True)
    for g in G + [Gb, Gc]:
        assert np.isfinite(g).all(), what
    nnz = sum(int(p.sum()) for _, _, _, p in rels if p is not None)
    cmax = max(ranks.values())
    assert ws < 64 * (nnz + sum(n.values()) * 4 * cmax + 8 * cmax * cmax) + n['t'] * n['b'] * 16 + (6 << 20), ws
    H5 = oracle_fold(rels, theta, ranks, Gp, S, G0, iters)
    Hb = oracle_fold(rels, theta, ranks, Gp, S2, G[iters], 1)
    Hc = oracle_fold(rels, theta, ranks, dict(Gp, a=Ga2), S2, Gb, 1)
    stages = [('after %d iterations' % iters, G[iters], H5), ('after set_backbone', Gb, Hb), ('after set_factor', Gc, Hc)]
    if dtype == 'f64':
        for name, got, want in stages:
            out[name] = within(relerr(got, want), 1e-9, '%s: list-fed f64 fold-in vs oracle, %s' % (what, name))
    else:
        Gd, _, Gbd, Gcd, _ = run(False)
        # (the re-preparation steps start from each plan's own state: the host steps from the same one)
        Hbd = oracle_fold(rels, theta, ranks, Gp, S2, Gd[iters], 1)
        Hcd = oracle_fold(rels, theta, ranks, dict(Gp, a=Ga2), S2, Gbd, 1)
        for (name, got, want), gd, wd in zip(stages, (Gd[iters], Gbd, Gcd), (H5, Hbd, Hcd)):
            yard = relerr(gd, wd)
            out[name] = (within(relerr(got, want), 2.0 * yard, '%s: list-fed vs f64 host (bound: 2 x the dense-fed plan\'s %.3e), %s'
                                % (what, yard, name)), yard)
    # relation_sqerr of the list-fed relations at the state after `iters` iterations
    Gt = G[iters]
    for k, (i, j, R, pat) in enumerate(rels):
        if pat is None:
            continue
        Sk = np.asarray(S[k], dtype=np.float64)
        if i == 't':
            r = sqerr_ratio(dtype, R, pat, Gt, Sk, Gp[j], sq[k], n['t'], n[j], ranks['t'], ranks[j])
        else:
            r = sqerr_ratio(dtype, R.T, pat.T, Gt, Sk.T, Gp[i], sq[k], n['t'], n[i], ranks['t'], ranks[i])
        out['sqerr %d' % k] = within(r, 1.0, '%s: relation_sqerr of relation %d (%s x %s), |delta| / model bound' % (what, k, i, j))
    return out


def zero_relation_case(dtype, ranks, what, n=None, seed=3):
    """An all-zero relation (nnz = 0) beside the others: finite factors, and its squared error is the trace term."""
    n = n or {'t': 131, 'a': 197, 'b': 90}
    rels, rs = fold_graph(n, seed, zero_first=True)
    assert int(rels[0][3].sum()) == 0
    Gp = {o: rs.rand(n[o], ranks[o]) + 0.1 for o in ('a', 'b')}
    S = [K.store_round(rs.rand(ranks[i], ranks[j]) * 2.0 - 0.6, 'f32') for i, j, _, _ in rels]
    G0 = rs.rand(n['t'], ranks['t']) + 0.1
    plan = make_plan(dtype, n, ranks, rels, None, Gp, S, G0, True)
    try:
        plan.iterate(3)
        Gt, Ga = plan.get_factor('t'), plan.get_factor('a')
        sq = plan.relation_sqerr(0)
    finally:
        plan.close()
    assert np.isfinite(Gt).all() and (Gt[7] >= 0).all(), what
    trace = np.sum((Gt @ S[0] @ Ga.T) ** 2)
    # the trace term alone: f64 c x c products of Gram matrices summed over n objects in f64
    within(abs(sq - trace) / trace, 1e-9, '%s: squared error of an all-zero relation vs tr(S^T Gram_t S Gram_a)' % what)


# ---- 4. flags and lists ------------------------------------------------------------------------------------------------
def create_status(lib, variant, flags, mask_ptr=None, n_rows=0, ranks=(8, 6), known=10, target=0):
    """Status of skf_plan_create for one 40 x 30 relation (no HIP call is made before the validation answers)."""
    rel = dict(row_type=0, col_type=1, flags=flags, known_bound=known, n_rows=n_rows)
    if mask_ptr is not None:
        rel.update(mask=mask_ptr, mask_ld=30)
    return plan_create_status(lib, [(40, ranks[0]), (30, ranks[1])], [rel], variant=variant,
                              target=target if variant == nat.SKF_TRANSFORM else -1)[0]


def creation_flag_cases(lib, mask_ptr):
    """The plan-creation checks that run before any HIP call: a non-transform plan, the flag with either CSR flag, a mask."""
    bad, F = nat.SKF_E_INVALID, nat.SKF_REL_FOLD_CSR
    assert create_status(lib, nat.SKF_TRANSFORM, F) == 0
    assert create_status(lib, nat.SKF_TRANSFORM, F, target=1) == 0
    assert create_status(lib, nat.SKF_DFMF, F) == bad
    assert create_status(lib, nat.SKF_DFMC, F) == bad
    assert create_status(lib, nat.SKF_TRANSFORM, F | nat.SKF_REL_KNOWN_CSR) == bad
    assert create_status(lib, nat.SKF_TRANSFORM, F | nat.SKF_REL_SPARSE_CSR) == bad
    assert create_status(lib, nat.SKF_TRANSFORM, F, mask_ptr=mask_ptr) == bad
    assert create_status(lib, nat.SKF_TRANSFORM, nat.SKF_REL_SPARSE_CSR) == bad         # (stays an error on fold-in plans)


def invalid_flag_cases():
    rt = nat.get_runtime()
    bad, F = nat.SKF_E_INVALID, nat.SKF_REL_FOLD_CSR
    creation_flag_cases(rt.lib, rt.mem.empty(4096).ptr)
    assert create_status(rt.lib, nat.SKF_TRANSFORM, F, n_rows=20) == bad                # a row block
    assert create_status(rt.lib, nat.SKF_TRANSFORM, F | nat.SKF_REL_ABSENT) == bad
    assert create_status(rt.lib, nat.SKF_TRANSFORM, F, ranks=(1025, 6)) == bad          # a rank above 1024
    assert create_status(rt.lib, nat.SKF_TRANSFORM, F, ranks=(8, 1025)) == bad
    assert create_status(rt.lib, nat.SKF_TRANSFORM, F, ranks=(1023, 6)) == 0            # (the largest rank any plan takes)
    assert create_status(rt.lib, nat.SKF_TRANSFORM, F, known=2000000001) == bad         # more than 2e9 entries
    assert create_status(rt.lib, nat.SKF_TRANSFORM, F, known=-1) == bad
    assert create_status(rt.lib, nat.SKF_TRANSFORM, F, known=0) == 0


def invalid_lists_case(kind, dtype='f64', by_col=False):
    """A broken list (the three edits of sparse_dfmf_cases.invalid_lists_case) or a missing hand-over is refused at bind."""
    rs = np.random.RandomState(5)
    n_a, n_b = 40, 30
    pat = rs.rand(n_a, n_b) < 0.2
    pat[0, :4] = True
    pat[:4, 0] = True
    ke = entries_along(np.where(pat, 1.0, 0.0), pat, by_col)
    n_in = n_a if by_col else n_b
    if kind == 'indptr':
        ke.indptr[5], ke.indptr[6] = ke.indptr[6], ke.indptr[5] - 1
    elif kind == 'column':
        ke.indices[2] = n_in
    elif kind == 'order':
        ke.indices[0], ke.indices[1] = ke.indices[1], ke.indices[0]
    ke.validate = lambda: None                      # (the host check of the engine is not what is tested here)
    types, n, ranks = ['a', 'b'], {'a': n_a, 'b': n_b}, {'a': 8, 'b': 6}
    target = 'b' if by_col else 'a'
    if kind == 'handover':
        rt = nat.get_runtime()
        tdesc = (nat.TypeDesc * 2)()
        tdesc[0].n_obj, tdesc[0].rank, tdesc[1].n_obj, tdesc[1].rank = n_a, 8, n_b, 6
        rdesc = (nat.RelationDesc * 1)()
        rdesc[0].row_type, rdesc[0].col_type = 0, 1
        rdesc[0].flags, rdesc[0].known_bound = nat.SKF_REL_FOLD_CSR, ke.known
        opt = nat.Options(nat.DTYPES[dtype], nat.SKF_TRANSFORM, 1 if by_col else 0, nat.SKF_ENGINE_MFMA, 0, 0, 0)
        handle = nat._P()
        rt.call('skf_plan_create', 2, tdesc, 1, rdesc, 0, (nat.ThetaDesc * 1)(), C.byref(opt), C.byref(handle))
        try:
            nbytes = C.c_size_t()
            rt.call('skf_plan_workspace_bytes', handle, C.byref(nbytes))
            ws = rt.mem.empty(nbytes.value)
            with pytest.raises(nat.SkfNativeError) as exc:
                rt.call('skf_plan_bind_workspace', handle, ws.ptr, nbytes.value, rt.mem.stream)
            assert exc.value.code == nat.SKF_E_INVALID
        finally:
            rt.lib.skf_plan_destroy(handle)
        return
    with pytest.raises(nat.SkfNativeError) as exc:
        DevicePlan(types, n, ranks, [('a', 'b', ke, None)], [], nat.SKF_TRANSFORM, dtype=dtype, target=target).close()
    assert exc.value.code == nat.SKF_E_INVALID
    # ... and the host layer refuses lists compressed along the wrong side before anything is created
    good = entries_along(np.where(pat, 1.0, 0.0), pat, not by_col)
    with pytest.raises(ValueError):
        DevicePlan(types, n, ranks, [('a', 'b', good, None)], [], nat.SKF_TRANSFORM, dtype=dtype, target=target).close()


def refusal_order_case(which):
    """A fold-in relation (SKF_REL_FOLD_CSR, lists along the target's 4 objects) with defective lists: refused by the
    validation kernel alone."""
    import known_csr_cases as KC
    KC.refused_after_one_launch(lambda w: KC.small_plan(w, nat.SKF_TRANSFORM, 'zero', target='a').close(), which)


# ---- 5. the public API -------------------------------------------------------------------------------------------------
def fitted(n_u, n_m, n_g, ranks, n_run=1, seed=1):
    """A small fitted model: users x movies and movies x genres, both dense, f64."""
    from skfusion_amd.fusion import FusionGraph, Relation, ObjectType, Dfmf
    rs = np.random.RandomState(seed)
    users, movies, genres = ObjectType('users', ranks[0]), ObjectType('movies', ranks[1]), ObjectType('genres', ranks[2])
    g = FusionGraph([Relation(rs.rand(n_u, n_m), users, movies, name='counts'),
                     Relation((rs.rand(n_m, n_g) < 0.3).astype(float), movies, genres, name='genres')])
    f = Dfmf(max_iter=3, init_type='random', random_state=2, dtype='f64', n_run=n_run).fuse(g)
    return f, (users, movies, genres)


def new_counts(shape, density, seed, fmt):
    """New objects' relation as scipy.sparse in `fmt`, COO triplets with a duplicate and a stored zero, values multiples of
    1/8 of both signs."""
    import scipy.sparse
    rs = np.random.RandomState(seed)
    k = max(int(density * shape[0] * shape[1]), 4)
    u, m = rs.randint(0, shape[0], k), rs.randint(0, shape[1], k)
    v = rs.randint(-31, 32, k) / 8.0
    u = np.concatenate([u, [0, 0, 2]])
    m = np.concatenate([m, [1, 1, 3]])
    v = np.concatenate([v, [0.25, 0.5, 0.0]])
    return getattr(scipy.sparse.coo_matrix((v, (u, m)), shape=shape), 'to' + fmt)()


def fold_api(fuser, target, rels, data, **kw):
    """DfmfTransform of `target` through `rels` = [(row type, col type)] carrying `data` (one matrix per relation)."""
    from skfusion_amd.fusion import FusionGraph, Relation, DfmfTransform
    g = FusionGraph([Relation(d, i, j) for (i, j), d in zip(rels, data)])
    args = dict(max_iter=4, init_type='random', random_state=4)
    args.update(kw)
    return DfmfTransform(**args).transform(target, g, fuser)


def api_host(fuser, target, rels, dense, iters, seed=4, run=0):
    """oracle.dfmf_oracle.transform of the same fold-in (init_type='random': G0 = RandomState(seed).rand(n, c))."""
    from oracle import dfmf_oracle as orc
    R, S = {}, {}
    for (i, j), d in zip(rels, dense):
        R[i, j] = [d]
        S[i, j] = [fuser.backbone([r for r in fuser.fusion_graph.relations if (r.row_type, r.col_type) == (i, j)][0], run)]
    G = {(t, t): fuser.factor(t, run) for t in fuser.fusion_graph.object_types}
    n_t = dense[0].shape[0 if rels[0][0] == target else 1]
    G0 = np.random.RandomState(seed).rand(n_t, int(target.rank))
    return orc.transform(R, {}, target, {t: int(t.rank) for t in G_types(G)}, G, S, max_iter=iters, G0=G0)


def G_types(G):
    return [t for t, _ in G]


def api_formats_case(dtype, fmts, monkeypatch, sizes=(60, 50, 12), ranks=(16, 12, 4), n_new=23, density=0.1):
    """sparse_relations=True on CSR / CSC / COO input for a row-side target (new users) and a column-side one (new movies,
    which also have a row-side relation): never expanded, and within the bounds of whole_case of the same DfmfTransform on
    toarray()."""
    import sparse_dfmf_api_cases as AC
    fuser, (users, movies, genres) = fitted(sizes[0], sizes[1], sizes[2], ranks)
    out = {}
    for fmt in fmts:
        for side, target, rels, shapes in (
                ('row', users, [(users, movies)], [(n_new, sizes[1])]),
                ('column', movies, [(users, movies), (movies, genres)], [(sizes[0], n_new), (n_new, sizes[2])])):
            sp = [new_counts(s, density, 11 + k, fmt) for k, s in enumerate(shapes)]
            dense = [m.toarray() for m in sp]
            spied = [AC.forbid_toarray(monkeypatch, m.copy()) for m in sp]
            a = fold_api(fuser, target, rels, spied, dtype=dtype, sparse_relations=True).factor(target)
            b = fold_api(fuser, target, rels, dense, dtype=dtype).factor(target)
            host = api_host(fuser, target, rels, dense, 4)
            what = 'DfmfTransform %s %s %s-side target' % (dtype, fmt, side)
            assert a.shape == (n_new, int(target.rank)) and np.isfinite(a).all()
            if dtype == 'f64':
                within(relerr(a, host), 1e-9, what + ': stored entries vs oracle')
                within(relerr(b, host), 1e-9, what + ': toarray() vs oracle')
            else:
                yard = relerr(b, host)
                out[what] = (within(relerr(a, host), 2.0 * yard, what + ': stored entries vs f64 host (bound: 2 x toarray()\'s)'), yard)
            # False: today's path, bit for bit; None below 2^20 cells: the same
            c = fold_api(fuser, target, rels, sp, dtype=dtype, sparse_relations=False).factor(target)
            d = fold_api(fuser, target, rels, sp, dtype=dtype).factor(target)
            assert np.array_equal(c, b) and np.array_equal(d, b), what
    return out


def api_rule_case(monkeypatch):
    """sparse_relations=None: 2048 x 1024 at density 1e-3 (2^21 cells, 1e-3 * 16 <= 4) takes the lists -- the spied matrix is
    never expanded --, the same relation at density 0.3 (0.3 * 16 > 4) is expanded."""
    import sparse_dfmf_api_cases as AC
    from skfusion_amd.fusion import Relation
    from skfusion_amd.fusion.decomposition.dfmf import fold_entries_apply
    fuser, (users, movies, genres) = fitted(40, 1024, 6, (16, 12, 4))
    sp = new_counts((2048, 1024), 1e-3, 21, 'csr')
    a = fold_api(fuser, users, [(users, movies)], [AC.forbid_toarray(monkeypatch, sp.copy())], max_iter=2).factor(users)
    b = fold_api(fuser, users, [(users, movies)], [sp.toarray()], max_iter=2).factor(users)
    within(relerr(a, b), 1e-9, 'DfmfTransform f64, default rule at 2048 x 1024: stored entries vs toarray()')
    assert fold_entries_apply(Relation(sp, users, movies), None)
    assert not fold_entries_apply(Relation(new_counts((2048, 1024), 0.3, 22, 'csr'), users, movies), None)
    assert not fold_entries_apply(Relation(new_counts((1023, 1024), 1e-3, 23, 'csr'), users, movies), None)       # < 2^20 cells
    assert not fold_entries_apply(Relation(sp, users, movies, preprocessor=lambda x: x), True)
    assert not fold_entries_apply(Relation(sp, users, movies, unstored='unknown'), True)
    assert not fold_entries_apply(Relation(new_counts((64, 64), 0.1, 24, 'csr'), users, users), True)


def api_runs_and_errors_case(monkeypatch):
    """n_run = 3 in shared launches against three single fold-ins; compute_err / stopping_system with a callback: as many
    iterations as the dense path and the same system error; init_type='random_c' and a stored non-finite value."""
    import logging
    import sparse_dfmf_api_cases as AC
    fuser, (users, movies, genres) = fitted(60, 50, 12, (16, 12, 4), n_run=3)
    sp = new_counts((23, 50), 0.1, 31, 'csr')
    rels = [(users, movies)]
    spy = lambda: [AC.forbid_toarray(monkeypatch, sp.copy())]
    batched = fold_api(fuser, users, rels, spy(), n_run=3, sparse_relations=True)
    singles = fold_api(fuser, users, rels, spy(), n_run=3, sparse_relations=True, callback=lambda G, it: None)
    for x, y in zip(batched.factor(users), singles.factor(users)):
        assert np.array_equal(x, y), 'n_run = 3: shared launches vs one fold-in after the other'

    class Grab(logging.Handler):
        def __init__(self):
            logging.Handler.__init__(self)
            self.errors = []

        def emit(self, record):
            if str(record.msg).startswith('Error (objective'):
                self.errors.append(float(record.args[0]))
    log = logging.getLogger('skfusion_amd')
    seen, errs = {}, {}
    for name, data, kw in (('lists', spy(), dict(sparse_relations=True)), ('dense', [sp.toarray()], {})):
        grab, its = Grab(), []
        old = (log.level, log.propagate)
        log.addHandler(grab)
        log.setLevel(logging.INFO)
        log.propagate = False
        try:
            fold_api(fuser, users, rels, data, max_iter=12, compute_err=True, stopping_system=1e-3,
                     callback=lambda G, it, its=its: its.append(it), **kw)
        finally:
            log.removeHandler(grab)
            log.setLevel(old[0])
            log.propagate = old[1]
        seen[name], errs[name] = its, np.array(grab.errors)
    assert seen['lists'] == seen['dense'] and len(seen['lists']) >= 3, seen
    # both are f64 evaluations of the same sums from factors that agree to 1e-9 (whole_case): the list form's own rounding
    # (sqerr_ratio's bound) is of the order (c + 2) 2^-53 of the sums it cancels, far below 1e-9 of the error here
    within(np.max(np.abs(errs['lists'] - errs['dense']) / errs['dense']), 1e-9, 'DfmfTransform f64: system error, stored entries vs toarray()')
    a = fold_api(fuser, users, rels, spy(), init_type='random_c', sparse_relations=True).factor(users)
    b = fold_api(fuser, users, rels, [sp.toarray()], init_type='random_c').factor(users)
    within(relerr(a, b), 1e-9, 'DfmfTransform f64 init_type=random_c: stored entries vs toarray()')
    # a stored NaN / inf takes fill_value, as `data[~isfinite] = fill_value` of the dense path; unstored entries stay zero
    bad = sp.copy().astype(float)
    bad.data[1], bad.data[4] = np.nan, np.inf
    a = fold_api(fuser, users, rels, [bad], fill_value=0.5, sparse_relations=True).factor(users)
    b = fold_api(fuser, users, rels, [bad.toarray()], fill_value=0.5).factor(users)
    assert np.isfinite(a).all()
    within(relerr(a, b), 1e-9, 'DfmfTransform f64, stored non-finite values take fill_value')
