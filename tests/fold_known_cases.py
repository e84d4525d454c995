"""Fold-ins on the KNOWN entries only (SKF_REL_FOLD_CSR | SKF_REL_FOLD_KNOWN, skf_fold_known_pass, fold_known_kernel in
csrc/skf_known.h, fusion.DfmcTransform) -- the SAME cases on the host emulator (small) and on the GPU.

The host model (`host_fold`) is the reference's own statement, dense and f64: the completion step of _dfmc.py:319-325 --
every unknown cell of a new relation takes the current model's prediction G_i S G_j^T -- followed by the target's update of
_dfmf.py:385-428, with every other factor and every backbone frozen.  The engine never forms the completed relation.

  1. skf_fold_known_pass bit for bit (pass_case).  G in {0, 1/2, 1}, T multiples of 1/4 in [-1, 1], v multiples of 1/8 in
     (-8, 8), X multiples of 1/32 in [-2, 2]: a prediction is a multiple of 1/8 of size <= c, a residual a multiple of 1/8
     below c + 8, an axpy term a multiple of 1/32, and the sum over at most 197 entries stays below (c + 8) * 32 * 197 <
     2^23 units of 1/32 at c = 1024 -- every partial sum is exact in f32 in ANY order, so the host loop needs no lane map.
     E / D are pre-filled with low-bit values so that the one final addition rounds; a sentinel sits behind column c.
  2. whole fold-ins (whole_case): f64 within 1e-9 of the host model (the project's standing fold-in bound, DESIGN.md
     section 3).  f32 / bf16 have no dense device path for a masked fold-in, so the yardstick is existing code: the
     dense-fed SKF_TRANSFORM plan of the same engine on the same relations with the unknown cells set to ZERO, its relative
     deviation taken from oracle.dfmf_oracle.transform on that data; the masked plan may deviate from ITS f64 host model
     by at most 4 x that -- one factor 2 because each entry rounds a dot product, a residual and an axpy where the dense
     product rounds one, the other the project's allowance for the same terms summed in another order.
  3. properties, 4. what it is for (planted data), 5. refusals: see the functions."""
import ctypes as C

import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, KnownEntries
from helpers import relerr, within
import known_cases as K
import sparse_foldin_cases as FC
from dense_cases import constraint

EPS = np.finfo(np.float64).eps


def _split(x):
    return np.maximum(x, 0.0), np.maximum(-x, 0.0)


# ---- the host model: dense f64, complete, then update ------------------------------------------------------------------
def host_fold(rels, theta, target, Gp, S, G0, iters, on_iter=None):
    """rels = [(i, j, R, known pattern or None)], Gp = {type: frozen factor}, S = one backbone per relation.  Returns the
    target factor after every iteration (index 0: G0) and the known-entry / whole-relation squared errors of every
    relation after every iteration."""
    G = np.array(G0, dtype=np.float64)
    Tp, Tn = _split(np.asarray(theta, dtype=np.float64)) if theta is not None else (None, None)
    out, errs = [G.copy()], []

    def model(k):
        i, j, _, _ = rels[k]
        Sk = np.asarray(S[k], dtype=np.float64)
        return G @ Sk @ Gp[j].T if i == target else Gp[i] @ Sk @ G.T

    for it in range(iters):
        E, D = np.zeros_like(G), np.zeros_like(G)
        for k, (i, j, R, pat) in enumerate(rels):
            Sk = np.asarray(S[k], dtype=np.float64)
            Rc = np.asarray(R, dtype=np.float64) if pat is None else np.where(pat, R, model(k))      # _dfmc.py:319-325
            if i == target:                                                                          # _dfmf.py:392-405
                Gj = Gp[j]
                t1p, t1n = _split(Rc @ (Gj @ Sk.T))
                t2p, t2n = _split(Sk @ (Gj.T @ (Gj @ Sk.T)))
            else:                                                                                    # _dfmf.py:407-419
                Gr = Gp[i]
                t1p, t1n = _split(Rc.T @ (Gr @ Sk))
                t2p, t2n = _split(Sk.T @ (Gr.T @ (Gr @ Sk)))
            E += t1p + G @ t2n
            D += t1n + G @ t2p
        if Tp is not None:                                                                           # _dfmf.py:421-425
            D += Tp @ G
            E += Tn @ G
        G = G * np.sqrt(E / np.maximum(D, EPS))
        out.append(G.copy())
        sq = []
        for k, (i, j, R, pat) in enumerate(rels):
            d2 = (np.asarray(R, dtype=np.float64) - model(k)) ** 2
            sq.append(float(d2.sum() if pat is None else d2[pat].sum()))
        errs.append(sq)
        if on_iter is not None:
            on_iter(it)
    return out, np.array(errs)


# ---- 1. the stand-alone operator ---------------------------------------------------------------------------------------
def host_pass(indptr, indices, values, G, Tm, X, E, D, c, dtype):
    """tmp1 = X + sum_k (v_k - <G[o], T[i_k]>) T[i_k] in the engine's type (every partial sum is exact for the test's
    values, whatever the order), then the one rounding addition into E / D."""
    E, D = E.copy(), D.copy()
    for o in range(len(indptr) - 1):
        idx = indices[int(indptr[o]):int(indptr[o + 1])]
        v = values[int(indptr[o]):int(indptr[o + 1])]
        rows = Tm[idx, :c]
        x = (rows @ G[o, :c]).astype(dtype)
        e = (v - x).astype(dtype)
        tmp = (e @ rows).astype(dtype) if len(idx) else np.zeros(c, dtype=dtype)
        if X is not None:
            tmp = (tmp + X[o, :c]).astype(dtype)
        E[o, :c] = E[o, :c] + np.maximum(tmp, dtype(0))
        D[o, :c] = D[o, :c] + np.maximum(-tmp, dtype(0))
    return E, D


def pass_case(n_out, n_partner, c, pattern, dtype, with_x, seed=0):
    rt = nat.get_runtime()
    T_ = np.float64 if dtype == 'f64' else np.float32
    rs = np.random.RandomState(seed + c)
    pat = K.edge_mask(n_out, n_partner, pattern, seed)
    lens = pat.sum(axis=1)
    if pattern == 'edges':
        assert (lens == 0).any() and (lens == 1).any(), 'an object with an empty list and one with a single entry'
    if pattern == 'full':
        assert (lens == n_partner).any(), 'an object holding every partner'
    vals = (rs.randint(-63, 64, size=pat.shape) / 8.0).astype(T_)
    indptr, indices, values = FC.lists_of(pat, vals)
    ldg, ldt, ldx, lde, ldd = c + 1, c + 3, c + 4, c + 5, c + 2
    G = (rs.randint(0, 3, size=(n_out, ldg)) / 2.0).astype(T_)
    Tm = (rs.randint(-4, 5, size=(n_partner, ldt)) / 4.0).astype(T_)
    X = (rs.randint(-64, 65, size=(n_out, ldx)) / 32.0).astype(T_) if with_x else None
    E = (rs.randint(1, 2 ** 20, size=(n_out, lde)) / float(2 ** 22)).astype(T_)
    D = (rs.randint(1, 2 ** 20, size=(n_out, ldd)) / float(2 ** 22)).astype(T_)
    E[:, c:] = -77.0
    D[:, c:] = -55.0
    keep = lambda a: rt.mem.from_host(a if a.size else np.zeros(1, dtype=a.dtype))
    bp, bi, bv, bg, bt, be, bd = keep(indptr), keep(indices), keep(values), keep(G), keep(Tm), keep(E), keep(D)
    bx = keep(X) if with_x else None
    rt.call('skf_fold_known_pass', nat.DTYPES[dtype], bp.ptr, bi.ptr, bv.ptr, n_out, bg.ptr, ldg, bt.ptr, ldt, c,
            bx.ptr if with_x else None, ldx if with_x else 0, be.ptr, lde, bd.ptr, ldd, rt.mem.stream)
    rt.mem.synchronize()
    gE, gD = rt.mem.to_host(be, E.shape, T_), rt.mem.to_host(bd, D.shape, T_)
    hE, hD = host_pass(indptr, indices, values, G, Tm, X, E, D, c, T_)
    what = 'skf_fold_known_pass %s %s n_out %d c %d X %s' % (dtype, pattern, n_out, c, with_x)
    assert (hE[:, :c] != E[:, :c]).any() and (hD[:, :c] != D[:, :c]).any(), what + ': both halves of the split must be hit'
    assert np.array_equal(gE[:, :c], hE[:, :c]), '%s: E differs from the host loop (max %.3e)' % (what, np.max(np.abs(gE - hE)))
    assert np.array_equal(gD[:, :c], hD[:, :c]), '%s: D differs from the host loop (max %.3e)' % (what, np.max(np.abs(gD - hD)))
    assert np.array_equal(gE[:, c:], E[:, c:]) and np.array_equal(gD[:, c:], D[:, c:]), what + ': memory past column c changed'
    if not with_x:                      # an object with an empty list and no addend: nothing is added to its rows
        for o in np.nonzero(lens == 0)[0]:
            assert np.array_equal(gE[o], E[o]) and np.array_equal(gD[o], D[o]), what


def pass_refusals():
    """SKF_E_INVALID of the operator: a dtype that is not f64 / f32, every null pointer but X, widths 0 and 1025, every
    short leading dimension (X's only when X is given)."""
    rt = nat.get_runtime()
    b = rt.mem.empty(4096).ptr
    st = rt.mem.stream
    bad = nat.SKF_E_INVALID

    def call(dt=nat.SKF_F32, c=4, p=None, ld=None, x=b):
        p = dict(dict(indptr=b, indices=b, values=b, G=b, T=b, E=b, D=b), **(p or {}))
        ld = dict(dict(g=c, t=c, x=c, e=c, d=c), **(ld or {}))
        return rt.lib.skf_fold_known_pass(dt, p['indptr'], p['indices'], p['values'], 0, p['G'], ld['g'], p['T'], ld['t'], c, x,
                                          ld['x'], p['E'], ld['e'], p['D'], ld['d'], st)
    assert call() == 0 and call(dt=nat.SKF_F64) == 0            # (no output object: nothing is read or launched)
    assert call(x=None, ld=dict(x=0)) == 0                      # X may be NULL, its ld is then ignored
    assert call(dt=nat.SKF_BF16) == bad
    for name in ('indptr', 'indices', 'values', 'G', 'T', 'E', 'D'):
        assert call(p={name: None}) == bad, name
    assert call(c=0) == bad and call(c=1025) == bad and call(c=1024) == 0
    for name in ('g', 't', 'x', 'e', 'd'):
        assert call(c=8, ld={name: 7}) == bad, name
    rt.mem.synchronize()


# ---- 2. / 3. whole fold-ins --------------------------------------------------------------------------------------------
def known_along(R, pat, by_col):
    """KnownEntries(unstored='unknown') of the entries `pat` marks, compressed along the rows or (by_col) the columns."""
    if by_col:
        p, i, v = FC.lists_of(pat.T, np.ascontiguousarray(R.T))
    else:
        p, i, v = FC.lists_of(pat, R)
    return KnownEntries(p, i, v, R.shape, unstored='unknown', by_col=by_col)


def make_plan(dtype, n, ranks, rels, theta, Gp, S, G0, known=True):
    """known: the relations with a pattern as their known entries (the rest unknown); False: as dense matrices (the
    yardstick: unknown cells hold what `rels` holds there, zero)."""
    rl = [(i, j, known_along(R, pat, by_col=(j == 't')) if (known and pat is not None) else R, None) for i, j, R, pat in rels]
    plan = DevicePlan(['t', 'a', 'b'], n, ranks, rl, [('t', theta)] if theta is not None else [], nat.SKF_TRANSFORM,
                      dtype=dtype, target='t')
    for o in ('a', 'b'):
        plan.set_factor(o, Gp[o])
    plan.set_factor('t', G0)
    for k, s in enumerate(S):
        plan.set_backbone(k, s)
    return plan


def sqerr_ratio(dtype, R_tp, pat_tp, Gt, T_exact, Gsrc, Ssrc, got):
    """|device - host| / (K_SAFE bound) of skf_relation_sqerr of a known-entry fold-in relation in target x partner
    orientation: the first-order bound of sparse_dfmf_cases.pass_case for a sum of squared residuals over the lists.  The
    pass gathers T = Gsrc Ssrc^T as the engine forms and stores it (known_cases.gathered_T: Tr and how far the device's may
    lie from it), x = <G_t[o], T[i]> over c_t terms in the master type, e = v - x rounded once, e^2 and the sum in f64."""
    et = 'f32' if dtype == 'bf16' else dtype                   # (the pass runs on the f32 masters in the bf16 engine)
    u = K.U_ACC[et]
    c_t = Gt.shape[1]
    Tr, dT = K.gathered_T(Gsrc, Ssrc, et)
    assert np.allclose(Tr, T_exact, rtol=1e-5, atol=1e-6)
    Gr = K.store_round(Gt, et)
    x = Gr @ Tr.T
    dx = (c_t + 2) * u * (np.abs(Gr) @ np.abs(Tr).T) + np.abs(Gr) @ dT.T
    e = R_tp - x
    host = float(np.sum((e ** 2)[pat_tp]))
    bound = np.sum((2.0 * np.abs(e) * (dx + u * np.abs(e)))[pat_tp]) + (int(pat_tp.sum()) + 8) * 2.0 ** -53 * host
    return abs(got - host) / (K.K_SAFE * bound)


def whole_case(dtype, ranks, with_theta, what, n=None, iters=10, seed=0):
    """`iters` iterations of three known-entry relations plus a dense one -- the layout of sparse_foldin_cases.fold_graph:
    the target on the row side of one relation and the column side of another, two relations of one pair, one object
    without an entry anywhere -- against the f64 host model; iterate(k) against k x iterate(1); skf_relation_sqerr of every
    relation of the plan; the refusals that need a bound plan.  Returns the measured deviations."""
    n = n or {'t': 131, 'a': 197, 'b': 90}
    rels, rs = FC.fold_graph(n, seed)
    f32 = (lambda a: K.store_round(a, 'f32')) if dtype != 'f64' else (lambda a: a)
    Gp = {o: f32(rs.rand(n[o], ranks[o]) + 0.1) for o in ('a', 'b')}
    S = [f32(rs.rand(ranks[i], ranks[j]) * 2.0 - 0.6) for i, j, _, _ in rels]
    G0 = f32(rs.rand(n['t'], ranks['t']) + 0.1)
    theta = constraint('csr', n['t'], rs) if with_theta else None
    out = {}
    plan = make_plan(dtype, n, ranks, rels, theta, Gp, S, G0)
    try:
        assert not plan.batchable(), what + ': a plan with a known-entry relation does not batch'
        arr = (nat._P * 1)(plan.handle)
        assert plan.rt.lib.skf_iterate_batch(arr, 1, 1, plan.stream) == nat.SKF_E_INVALID, what
        assert b'SKF_REL_FOLD_KNOWN' in plan.rt.lib.skf_last_error()
        G, sq = [plan.get_factor('t')], []
        for _ in range(iters):
            plan.iterate(1)
            G.append(plan.get_factor('t'))
            sq.append([plan.relation_sqerr(k) for k in range(len(rels))])
        plan.set_factor('t', G0)
        plan.iterate(iters)
        np.testing.assert_array_equal(plan.get_factor('t'), G[iters], err_msg='%s: iterate(%d) vs %d x iterate(1)' % (what, iters, iters))
        with pytest.raises(nat.SkfNativeError) as exc:
            plan.get_contraction(0, 0)
        assert exc.value.code == nat.SKF_E_INVALID
        for device_init in (lambda: plan.relation_norms(0), lambda: plan.init_column_means('t', [(0, np.zeros((ranks['t'], 1), np.int32))])):
            with pytest.raises(nat.SkfNativeError) as exc:
                device_init()
            assert exc.value.code == nat.SKF_E_INVALID
        ws = plan.workspace_bytes
    finally:
        plan.close()
    for g in G:
        assert np.isfinite(g).all(), what
    nnz = sum(int(p.sum()) for _, _, _, p in rels if p is not None)
    cmax = max(ranks.values())
    assert ws < 64 * (nnz + sum(n.values()) * 4 * cmax + 8 * cmax * cmax) + n['t'] * n['b'] * 16 + (6 << 20), ws
    H, herr = host_fold(rels, theta, 't', Gp, S, G0, iters)
    dev = relerr(G[iters], H[iters])
    if dtype == 'f64':
        out['G'] = within(dev, 1e-9, '%s: known-entry f64 fold-in vs the f64 host model after %d iterations' % (what, iters))
    else:
        dense = make_plan(dtype, n, ranks, rels, theta, Gp, S, G0, known=False)
        try:
            dense.iterate(iters)
            Gd = dense.get_factor('t')
        finally:
            dense.close()
        yard = relerr(Gd, FC.oracle_fold(rels, theta, ranks, Gp, S, G0, iters))
        out['G'] = (within(dev, 4.0 * yard, '%s: known-entry fold-in vs its f64 host model after %d iterations (bound: 4 x the '
                           'zero-filled dense-fed plan\'s %.3e)' % (what, iters, yard)), yard)
    # skf_relation_sqerr of every relation at the state after each iteration: the known-entry objective of the three
    # known-entry relations at first order (state after the last iteration: the device's own factor), and, in f64, the
    # host model's errors of every iteration
    Gt = G[iters]
    for k, (i, j, R, pat) in enumerate(rels):
        if pat is None:
            continue
        Sk = np.asarray(S[k], dtype=np.float64)
        if i == 't':
            r = sqerr_ratio(dtype, R, pat, Gt, Gp[j] @ Sk.T, Gp[j], Sk, sq[-1][k])
        else:
            r = sqerr_ratio(dtype, R.T, pat.T, Gt, Gp[i] @ Sk, Gp[i], Sk.T, sq[-1][k])
        out['sqerr %d' % k] = within(r, 1.0, '%s: relation_sqerr of known-entry relation %d (%s x %s), |delta| / model bound' % (what, k, i, j))
    if dtype == 'f64':
        sq = np.array(sq)
        known = [k for k, r in enumerate(rels) if r[3] is not None]
        within(np.max(np.abs(sq[:, known] - herr[:, known]) / herr[:, known]), 1e-8,
               '%s: known-entry errors of every iteration vs the host model' % what)
    return out


def all_known_case(dtype, ranks, what, n=None, iters=6, seed=2):
    """Every entry known: nothing is completed, and the fold-in is the plain fold-in of the same dense relations (1e-9)."""
    n = n or {'t': 131, 'a': 197, 'b': 90}
    rels, rs = FC.fold_graph(n, seed)
    rels = [(i, j, R, None if pat is None else np.ones_like(pat)) for i, j, R, pat in rels]
    Gp = {o: rs.rand(n[o], ranks[o]) + 0.1 for o in ('a', 'b')}
    S = [rs.rand(ranks[i], ranks[j]) * 2.0 - 0.6 for i, j, _, _ in rels]
    G0 = rs.rand(n['t'], ranks['t']) + 0.1
    got = []
    for known in (True, False):
        plan = make_plan(dtype, n, ranks, rels, None, Gp, S, G0, known=known)
        try:
            plan.iterate(iters)
            got.append(plan.get_factor('t'))
        finally:
            plan.close()
    within(relerr(got[0], got[1]), 1e-9, '%s: every entry known vs the plain fold-in of the dense relations' % what)
    within(relerr(got[0], FC.oracle_fold(rels, None, ranks, Gp, S, G0, iters)), 1e-9, '%s: every entry known vs oracle.transform' % what)


def monotone_case(dtype, ranks, what, n=None, iters=20, seed=4):
    """The known-entry error of every known-entry relation's SUM does not increase over 20 iterations (f64; the frozen
    backbones are non-negative and mixed-sign in turn)."""
    n = n or {'t': 131, 'a': 197, 'b': 90}
    rels, rs = FC.fold_graph(n, seed)
    rels = rels[:1]                                     # one relation: its known-entry objective is what the update descends
    for signed in (False, True):
        Gp = {o: rs.rand(n[o], ranks[o]) + 0.1 for o in ('a', 'b')}
        S = [rs.rand(ranks[i], ranks[j]) - (0.3 if signed else 0.0) for i, j, _, _ in rels]
        G0 = rs.rand(n['t'], ranks['t']) + 0.1
        plan = make_plan(dtype, n, ranks, rels, None, Gp, S, G0)
        try:
            errs = []
            for _ in range(iters):
                plan.iterate(1)
                errs.append(plan.relation_sqerr(0))
        finally:
            plan.close()
        errs = np.array(errs)
        assert np.isfinite(errs).all() and (np.diff(errs) <= 1e-12 * errs[:-1]).all(), '%s signed %s: %r' % (what, signed, errs)
        _, herr = host_fold(rels, None, 't', Gp, S, G0, iters)
        within(np.max(np.abs(errs - herr[:, 0]) / herr[:, 0]), 1e-8, '%s signed %s: known-entry error of every iteration vs host' % (what, signed))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def creation_flag_cases(lib):
    """SKF_E_INVALID of skf_plan_create, before any HIP call: the flag without SKF_REL_FOLD_CSR, on SKF_DFMF / SKF_DFMC
    plans; every refusal SKF_REL_FOLD_CSR has stays (with the new flag too)."""
    bad, F, KN = nat.SKF_E_INVALID, nat.SKF_REL_FOLD_CSR, nat.SKF_REL_FOLD_KNOWN
    assert KN == 1024
    assert FC.create_status(lib, nat.SKF_TRANSFORM, F | KN) == 0
    assert FC.create_status(lib, nat.SKF_TRANSFORM, F | KN, target=1) == 0
    assert FC.create_status(lib, nat.SKF_TRANSFORM, KN) == bad
    assert b'SKF_REL_FOLD_KNOWN' in lib.skf_last_error()
    for variant in (nat.SKF_DFMF, nat.SKF_DFMC):
        assert FC.create_status(lib, variant, F | KN) == bad
        assert FC.create_status(lib, variant, KN) == bad
        assert b'SKF_REL_FOLD_KNOWN' in lib.skf_last_error()
    assert FC.create_status(lib, nat.SKF_TRANSFORM, F | KN | nat.SKF_REL_KNOWN_CSR) == bad
    assert FC.create_status(lib, nat.SKF_TRANSFORM, F | KN | nat.SKF_REL_SPARSE_CSR) == bad
    assert FC.create_status(lib, nat.SKF_TRANSFORM, F | nat.SKF_REL_KNOWN_CSR) == bad
    assert FC.create_status(lib, nat.SKF_TRANSFORM, F | nat.SKF_REL_SPARSE_CSR) == bad
    assert FC.create_status(lib, nat.SKF_TRANSFORM, nat.SKF_REL_KNOWN_CSR) == bad
    assert lib.skf_abi_version() == 5


def invalid_flag_cases():
    rt = nat.get_runtime()
    bad, F = nat.SKF_E_INVALID, nat.SKF_REL_FOLD_CSR | nat.SKF_REL_FOLD_KNOWN
    creation_flag_cases(rt.lib)
    assert FC.create_status(rt.lib, nat.SKF_TRANSFORM, F, mask_ptr=rt.mem.empty(4096).ptr) == bad
    assert FC.create_status(rt.lib, nat.SKF_TRANSFORM, F, n_rows=20) == bad                # a row block
    assert FC.create_status(rt.lib, nat.SKF_TRANSFORM, F | nat.SKF_REL_ABSENT) == bad
    assert FC.create_status(rt.lib, nat.SKF_TRANSFORM, F, ranks=(1025, 6)) == bad          # a rank above 1024
    assert FC.create_status(rt.lib, nat.SKF_TRANSFORM, F, ranks=(8, 1025)) == bad
    assert FC.create_status(rt.lib, nat.SKF_TRANSFORM, F, known=2000000001) == bad         # more than 2e9 entries
    assert FC.create_status(rt.lib, nat.SKF_TRANSFORM, F, known=-1) == bad
    assert FC.create_status(rt.lib, nat.SKF_TRANSFORM, F, known=0) == 0


def invalid_lists_case(kind, dtype='f64', by_col=False):
    """A broken list (the three edits of sparse_foldin_cases.invalid_lists_case) or a missing hand-over is refused at bind."""
    rs = np.random.RandomState(5)
    n_a, n_b = 40, 30
    pat = rs.rand(n_a, n_b) < 0.2
    pat[0, :4] = True
    pat[:4, 0] = True
    ke = known_along(np.where(pat, 1.0, 0.0), pat, by_col)
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
        rdesc[0].flags, rdesc[0].known_bound = nat.SKF_REL_FOLD_CSR | nat.SKF_REL_FOLD_KNOWN, ke.known
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
    good = known_along(np.where(pat, 1.0, 0.0), pat, not by_col)
    with pytest.raises(ValueError):
        DevicePlan(types, n, ranks, [('a', 'b', good, None)], [], nat.SKF_TRANSFORM, dtype=dtype, target=target).close()


# ---- the public API ------------------------------------------------------------------------------------------------------
def new_ratings(shape, density, seed, fmt):
    """New objects' relation with unknown cells as scipy.sparse in `fmt`: distinct cells (no duplicates: every format
    holds the same entries), a stored zero among them, values multiples of 1/8 of both signs; object 0 holds no entry."""
    import scipy.sparse
    rs = np.random.RandomState(seed)
    pat = rs.rand(*shape) < density
    pat[0, :] = False
    pat[:, 0] = False
    pat[1, 1] = pat[2, 3] = True
    vals = rs.randint(-31, 32, size=shape) / 8.0
    vals[2, 3] = 0.0
    u, m = np.nonzero(pat)
    order = rs.permutation(u.size)                  # (triplets in no particular order)
    return getattr(scipy.sparse.coo_matrix((vals[u, m][order], (u[order], m[order])), shape=shape), 'to' + fmt)(), vals, pat


def fold_known_api(fuser, target, rels, data, cls=None, unstored='unknown', **kw):
    """DfmcTransform (or `cls`) of `target` through `rels` = [(row type, col type)] carrying `data`."""
    from skfusion_amd.fusion import FusionGraph, Relation, DfmcTransform
    import scipy.sparse
    g = FusionGraph([Relation(d, i, j, **(dict(unstored=unstored) if scipy.sparse.issparse(d) else {})) for (i, j), d in zip(rels, data)])
    args = dict(max_iter=4, init_type='random', random_state=4)
    args.update(kw)
    return (cls or DfmcTransform)(**args).transform(target, g, fuser)


def api_model(fuser, target, rels, run=0):
    """(Gp, S) of the fitted model for `rels`: the frozen factors by type and one backbone per new relation."""
    Gp = {t: fuser.factor(t, run) for t in fuser.fusion_graph.object_types}
    S = [fuser.backbone([r for r in fuser.fusion_graph.relations if (r.row_type, r.col_type) == (i, j)][0], run) for i, j in rels]
    return Gp, S


def api_formats_case(dtype, fmts, monkeypatch, sizes=(60, 50, 12), ranks=(16, 12, 4), n_new=23, density=0.15):
    """Relation(scipy.sparse, unstored='unknown') in csr / csc / coo for a row-side target (new users) and a column-side one
    (new movies, which also have a dense row-side relation): never expanded, equal bits whatever the format, equal bits for
    the MaskedArray of the same cells, and (f64) within 1e-9 of the host model."""
    import sparse_dfmf_api_cases as AC
    fuser, (users, movies, genres) = FC.fitted(sizes[0], sizes[1], sizes[2], ranks)
    for side, target, rels, shapes in (
            ('row', users, [(users, movies)], [(n_new, sizes[1])]),
            ('column', movies, [(users, movies), (movies, genres)], [(sizes[0], n_new), (n_new, sizes[2])])):
        got = {}
        for fmt in fmts:
            sp, vals, pat = new_ratings(shapes[0], density, 11, fmt)
            extra = [np.random.RandomState(12).rand(*s) for s in shapes[1:]]
            data = [AC.forbid_toarray(monkeypatch, sp.copy())] + extra
            got[fmt] = fold_known_api(fuser, target, rels, data, dtype=dtype).factor(target)
            assert got[fmt].shape == (n_new, int(target.rank)) and np.isfinite(got[fmt]).all()
        what = 'DfmcTransform %s %s-side target' % (dtype, side)
        for fmt in fmts[1:]:
            assert np.array_equal(got[fmt], got[fmts[0]]), '%s: %s vs %s' % (what, fmt, fmts[0])
        ma = np.ma.MaskedArray(vals, mask=~pat)
        g_ma = fold_known_api(fuser, target, rels, [ma] + extra, dtype=dtype).factor(target)
        assert np.array_equal(g_ma, got[fmts[0]]), what + ': MaskedArray vs scipy.sparse with unstored=\'unknown\''
        if dtype == 'f64':
            Gp, S = api_model(fuser, target, rels)
            hr = [(rels[0][0], rels[0][1], np.where(pat, vals, 0.0), pat)] + [(i, j, d, None) for (i, j), d in zip(rels[1:], extra)]
            G0 = np.random.RandomState(4).rand(n_new, int(target.rank))
            H, _ = host_fold(hr, None, target, Gp, S, G0, 4)
            within(relerr(got[fmts[0]], H[4]), 1e-9, what + ': known entries vs the f64 host model')
            # ... and DfmfTransform is unchanged: it still expands and fills (another model, another factor)
            from skfusion_amd.fusion import DfmfTransform
            filled = fold_known_api(fuser, target, rels, [sp.copy()] + extra, cls=DfmfTransform, dtype=dtype).factor(target)
            dense0 = fold_known_api(fuser, target, rels, [np.where(pat, vals, 0.0)] + extra, cls=DfmfTransform, dtype=dtype).factor(target)
            assert np.array_equal(filled, dense0) and not np.allclose(filled, got[fmts[0]]), what


def api_no_unknown_case(monkeypatch):
    """A graph without an unknown cell: DfmcTransform returns DfmfTransform's factor, bit for bit -- an ndarray, a
    MaskedArray that masks nothing, unstored='zero' dense-fed and list-fed (`sparse_relations`)."""
    from skfusion_amd.fusion import DfmfTransform
    fuser, (users, movies, genres) = FC.fitted(60, 50, 12, (16, 12, 4))
    rels = [(users, movies)]
    sp = FC.new_counts((23, 50), 0.1, 31, 'csr')
    dense = sp.toarray()
    for name, data, kw in (('ndarray', dense, {}), ('unmasked MaskedArray', np.ma.MaskedArray(dense, mask=False), {}),
                           ('unstored=zero', sp, dict(unstored='zero')),
                           ('unstored=zero as lists', sp, dict(unstored='zero', sparse_relations=True))):
        a = fold_known_api(fuser, users, rels, [data], init_type='random_c', **kw).factor(users)
        b = fold_known_api(fuser, users, rels, [data], cls=DfmfTransform, init_type='random_c', **kw).factor(users)
        assert np.array_equal(a, b), 'DfmcTransform vs DfmfTransform, no unknown cell: ' + name


def api_restarts_stopping_and_fill_case():
    """n_run = 2: each restart's own fold-in; stopping_system stops where the host model driven by the same rule stops
    (the KNOWN-ENTRY objective); a stored non-finite value is unknown; fill_value reaches the initialiser only; a
    preprocessor on a relation with unknown cells raises DataFusionError."""
    from skfusion_amd.fusion import FusionGraph, Relation, DfmcTransform, DataFusionError
    fuser, (users, movies, genres) = FC.fitted(60, 50, 12, (16, 12, 4), n_run=2)
    rels = [(users, movies)]
    sp, vals, pat = new_ratings((23, 50), 0.2, 31, 'csr')
    R0 = np.where(pat, vals, 0.0)
    both = fold_known_api(fuser, users, rels, [sp.copy()], n_run=2)
    # (G0 of restart k is drawn k-th from the one RandomState, as the per-restart calls would draw)
    draw = np.random.RandomState(4)
    for run in range(2):
        Gp, S = api_model(fuser, users, rels, run)
        G0 = draw.rand(23, int(users.rank))
        H, _ = host_fold([(users, movies, R0, pat)], None, users, Gp, S, G0, 4)
        within(relerr(both.factor(users, run), H[4]), 1e-9, 'DfmcTransform n_run = 2: restart %d vs the host model of ITS frozen model' % run)
    assert not np.allclose(both.factor(users, 0), both.factor(users, 1))
    # stopping_system: previous - current system error < tol, read before iteration it > 1 (_dfmf.py:367-376, 433-450)
    Gp, S = api_model(fuser, users, rels, 0)
    G0 = np.random.RandomState(4).rand(23, int(users.rank))
    _, herr = host_fold([(users, movies, R0, pat)], None, users, Gp, S, G0, 40)
    s = np.sqrt(herr[:, 0])
    drops = s[:-1] - s[1:]
    tol = float(np.sqrt(drops[6] * drops[7]))            # between two consecutive drops of the host's own sequence
    want = next((it for it in range(2, 40) if s[it - 2] - s[it - 1] < tol), 40)
    assert 2 < want < 40 and abs(drops[want - 2] - tol) > 1e-6 * tol, (want, tol)
    its = []
    fold_known_api(fuser, users, rels, [sp.copy()], max_iter=40, stopping_system=tol, callback=lambda G, it: its.append(it))
    assert its == list(range(want)), 'stopping_system: %r iterations, the host model driven by the same rule runs %d' % (its, want)
    # a stored NaN / inf is unknown: the same fold-in as without the two cells
    bad = sp.copy().astype(float)
    bad.data[1], bad.data[4] = np.nan, np.inf
    keep = np.ones(sp.data.size, dtype=bool)
    keep[[1, 4]] = False
    import scipy.sparse
    coo = sp.tocoo()
    fewer = scipy.sparse.coo_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=sp.shape).tocsr()
    a = fold_known_api(fuser, users, rels, [bad], fill_value=0.5).factor(users)
    b = fold_known_api(fuser, users, rels, [fewer], fill_value=0.5).factor(users)
    assert np.isfinite(a).all() and np.array_equal(a, b), 'stored non-finite values are unknown'
    # fill_value: read by the initialiser only ('random' never reads the relation: no trace of it; 'random_c' forms its
    # column means over it, exactly as DfmfTransform's initialiser sees the filled matrix -- same draws, same G0)
    a = fold_known_api(fuser, users, rels, [sp.copy()], fill_value=0.5).factor(users)
    b = fold_known_api(fuser, users, rels, [sp.copy()], fill_value=-3.0).factor(users)
    assert np.array_equal(a, b)
    from skfusion_amd.fusion.decomposition._init import initialize
    from skfusion_amd.fusion.decomposition.dfmc import known_lists
    rel = Relation(sp.copy(), users, movies, unstored='unknown')
    ke = known_lists(rel, False, 0.5)
    filled = np.where(pat, vals, 0.5)
    rank = {users: int(users.rank)}
    for init_type in ('random_c', 'random_vcol'):
        g_l = initialize([users], {users: 23}, rank, {(users, movies): ke}, init_type, np.random.RandomState(7))[users, users]
        g_d = initialize([users], {users: 23}, rank, {(users, movies): filled}, init_type, np.random.RandomState(7))[users, users]
        within(relerr(g_l, g_d), 1e-12, 'DfmcTransform %s over the lists vs over the filled matrix' % init_type)
    # a preprocessor and unknown cells
    g = FusionGraph([Relation(sp.copy(), users, movies, unstored='unknown', preprocessor=lambda x: x)])
    with pytest.raises(DataFusionError):
        DfmcTransform(max_iter=2, init_type='random', random_state=4).transform(users, g, fuser)
    g = FusionGraph([Relation(np.ma.MaskedArray(vals, mask=~pat), users, movies, preprocessor=lambda x: x)])
    with pytest.raises(DataFusionError):
        DfmcTransform(max_iter=2, init_type='random', random_state=4).transform(users, g, fuser)


# ---- 4. what it is for -------------------------------------------------------------------------------------------------
class FrozenModel(object):
    """What a transformer reads of a fitted model: the object types, the relations, one factor per type and one backbone
    per relation (run 0) -- here the TRUE partner factor and backbone of planted data."""

    def __init__(self, graph, factors, backbones, init_type='random'):
        self.fusion_graph, self._G, self._S, self.init_type = graph, factors, backbones, init_type

    def factor(self, object_type, run=0):
        return self._G[object_type]

    def backbone(self, relation, run=0):
        return self._S[relation]


def planted_case(known_share, seed=0):
    """Planted data (120 new x 300 partners, ranks 8 / 6, noise 0.01, the true partner factor and backbone frozen), f64,
    100 iterations: the held-out RMSE of DfmcTransform is below the smaller of DfmfTransform's with fill_value = 0 and
    with the mean of the known entries.  Returns (masked, zero fill, mean fill)."""
    from skfusion_amd.fusion import FusionGraph, Relation, ObjectType, DfmcTransform, DfmfTransform
    import scipy.sparse
    rs = np.random.RandomState(seed)
    nt, n_p, ct, cp = 120, 300, 8, 6
    new, old = ObjectType('new', ct), ObjectType('old', cp)
    Gp, Gt = rs.rand(n_p, cp), rs.rand(nt, ct)
    S = rs.rand(ct, cp)
    R = Gt @ S @ Gp.T + 0.01 * rs.randn(nt, n_p)
    pat = rs.rand(nt, n_p) < known_share
    pat[7] = False
    fitted_rel = Relation(np.zeros((1, n_p)), new, old)          # (stands for the relation the model was fitted on)
    model = FrozenModel(FusionGraph([fitted_rel]), {new: None, old: Gp}, {fitted_rel: S})
    u, m = np.nonzero(pat)
    sp = scipy.sparse.coo_matrix((R[u, m], (u, m)), shape=R.shape).tocsr()
    kw = dict(max_iter=100, init_type='random', random_state=1, dtype='f64')
    ma = np.ma.MaskedArray(R, mask=~pat)
    g_c = DfmcTransform(**kw).transform(new, FusionGraph([Relation(sp, new, old, unstored='unknown')]), model).factor(new)
    g_0 = DfmfTransform(fill_value=0, **kw).transform(new, FusionGraph([Relation(ma, new, old)]), model).factor(new)
    g_m = DfmfTransform(fill_value=float(R[pat].mean()), **kw).transform(new, FusionGraph([Relation(ma, new, old)]), model).factor(new)
    rmse = lambda G: float(np.sqrt((((R - G @ S @ Gp.T) ** 2)[~pat]).mean()))
    out = rmse(g_c), rmse(g_0), rmse(g_m)
    print('planted data, %d %% known: held-out RMSE DfmcTransform %.4f, DfmfTransform zero fill %.4f, mean fill %.4f'
          % (round(100 * known_share), out[0], out[1], out[2]))
    assert out[0] < min(out[1], out[2]), out
    return out
