"""DFMF on relations given as the CSR of their stored entries, every other entry zero (SKF_REL_SPARSE_CSR,
csrc/skf_known.h + sparse_pass in csrc/skf_stages.inc) -- the SAME cases on the host emulator (small) and on the GPU.

First half: one valued pass P = R G_j, one Q = R^T G_i and one error pass held to a host model (pass_case).
  * f64 / f32: the factors are set to values of few bits (multiples of 1/256) and the stored values are multiples of 1/8,
    so every product r * g is exact in the engine's type and a fused multiply-add gives the bits of a multiply and an
    add; what is left is the ORDER of the additions, which the model repeats: lane groups of srp_vec_kernel walking a
    batch of 64 entries SRP_U steps at a time, the butterfly over the groups, the parts summed first to last
    (srp_any_kernel: one entry after the other).  np.array_equal.
  * bf16 rows: the model of known_cases.ones_case for the same kernel family -- f32 sums of exact products,
    |delta| <= K_SAFE (L + parts + 2) u (|R| |G|) element-wise, an empty list exactly 0.
  * error pass (every engine): its dot products x = <(G_i S)[row], G_j[col]> are not exact and G_i S comes off the
    matrix cores, so no host order reproduces the bits; first-order bound as known_cases.list_case derives it for
    SRP_ERR: sum over the stored entries of 2 (|r - x| + |x|) dx + 4 u ((r - x)^2 + x^2), dx = (c_j + 2) u |H| |G_j|^T
    + dH |G_j|^T (dH: the rounding of H = G_i S to the gathered type, known_cases.gathered_T; the bf16 engine gathers
    its f32 masters in this pass, so its model is the f32 one), plus the f64 rounding of
    the trace term tr(S^T Gram_i S Gram_j), (n_i + n_j + 2 (c_i + c_j)) 2^-53 sum (|G_i| |S| |G_j|^T)^2; times K_SAFE.
Second half: the lists a bind builds against scipy.sparse, invalid lists, whole fits against the dense-fed plan and the oracle."""
import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, KnownEntries
from helpers import plan_create_status, relerr, within
import known_cases as K


def stored_entries(R, pattern=None):
    """Dense matrix -> KnownEntries(unstored='zero') of the entries `pattern` marks (default: the non-zeros)."""
    R = np.asarray(R, dtype=np.float64)
    pat = (R != 0) if pattern is None else np.asarray(pattern, dtype=bool)
    rows, cols = np.nonzero(pat)                        # row-major: columns ascending within a row
    indptr = np.zeros(R.shape[0] + 1, dtype=np.int64)
    np.cumsum(pat.sum(axis=1), out=indptr[1:])
    return KnownEntries(indptr, cols, R[rows, cols], R.shape, unstored='zero')


def eighths(rs, shape):
    """Multiples of 1/8 in (0, 8): exact in bf16, so the dense bf16 copy of a relation holds them unrounded."""
    return rs.randint(1, 64, size=shape) / 8.0


# ---- host model of one valued pass ------------------------------------------------------------------------------------
def _vec_lanes(w, dtype):
    """GL of srp_vec_kernel as launch_srp picks it (16-byte chunks), 0: srp_any_kernel."""
    ve = 2 if dtype == 'f64' else 4
    gl = w // ve if w % ve == 0 else 0
    return gl if gl in (8, 16, 32, 64) else 0


def model_pass(indptr, indices, values, F, n_out, parts, part_w, dtype):
    """out[o] = sum over the entries (o, i, r) of r * F[i] in the kernels' own order and precision (f64 / f32)."""
    T = np.float64 if dtype == 'f64' else np.float32
    F = np.asarray(F, dtype=T)
    vals = np.asarray(values, dtype=T)
    w = F.shape[1]
    gl = _vec_lanes(w, dtype)
    out = np.zeros((n_out, w), dtype=T)
    for o in range(n_out):
        a, b = int(indptr[o]), int(indptr[o + 1])
        cols = indices[a:b]
        total = None
        for p in range(parts):
            sel = np.arange(a, b)[(cols >= p * part_w) & (cols < (p + 1) * part_w)] if parts > 1 else np.arange(a, b)
            if gl == 0:
                acc = np.zeros(w, dtype=T)
                for q in sel:
                    acc = acc + vals[q] * F[indices[q]]
            else:
                epw = 64 // gl
                grp = np.zeros((epw, w), dtype=T)
                for q0 in range(0, len(sel), 64):
                    batch = sel[q0:q0 + 64]
                    nb = len(batch)
                    for s0 in range(0, nb, epw * 4):
                        for u in range(4):
                            if s0 + u * epw >= nb:
                                break
                            for g in range(epw):
                                ent = s0 + u * epw + g
                                if ent < nb:
                                    q = batch[ent]
                                    grp[g] = grp[g] + vals[q] * F[indices[q]]
                off = 1
                while off < epw:                        # the butterfly over the lane groups: every group adds its partner's sum
                    grp = grp + grp[np.arange(epw) ^ off]
                    off *= 2
                acc = grp[0]
            total = acc if total is None else total + acc
        out[o] = total
    return out


def low_bit_factor(rs, n, c, bits):
    """Entries k / 2^bits in [1 / 2^bits, 1]: products with multiples of 1/8 below 8 stay exact in f32."""
    return rs.randint(1, 2 ** bits + 1, size=(n, c)) / float(2 ** bits)


def pass_case(n_a, n_b, c_a, c_b, dtype, parts, pattern, what, monkeypatch, seed=0, lengths=K.LIST_LENGTHS):
    """One a x b relation as stored entries (`pattern`: known_cases.edge_mask), DFMF on the engine `dtype`, lists in `parts`
    parts: P and Q of the first iteration (formed from G0) against the host model, then the squared error of the fitted
    state against the host's.  Returns the measured figures."""
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    rs = np.random.RandomState(seed)
    pat = K.edge_mask(n_a, n_b, pattern, seed, lengths)
    R = np.where(pat, eighths(rs, (n_a, n_b)), 0.0)
    ke = stored_entries(R, pat)
    bits = 6 if dtype == 'bf16' else 8                  # (bf16 holds 8 significant bits: k / 64 <= 1 is exact)
    G0 = {'a': low_bit_factor(rs, n_a, c_a, bits), 'b': low_bit_factor(rs, n_b, c_b, bits)}
    types, n, ranks = ['a', 'b'], {'a': n_a, 'b': n_b}, {'a': c_a, 'b': c_b}
    plan = DevicePlan(types, n, ranks, [('a', 'b', ke, None)], [], nat.SKF_DFMF, dtype=dtype)
    try:
        for t in types:
            plan.set_factor(t, G0[t])
        plan.set_profiling(True)
        plan.iterate(1)
        prof = plan.get_profile()
        plan.set_profiling(False)
        P = plan.get_contraction(0, 0)
        Q = plan.get_contraction(0, 1)
        S = plan.get_backbone(0).astype(np.float64)
        Gi, Gj = plan.get_factor('a').astype(np.float64), plan.get_factor('b').astype(np.float64)
        sq = plan.relation_sqerr(0)
        ws = plan.workspace_bytes
    finally:
        plan.close()
    nnz = int(pat.sum())
    out = {}
    # what a list pass executes: 2 nnz c flops; index + value lists and one gathered row per entry
    esz = {'f64': 8, 'f32': 4, 'bf16': 4}[dtype]
    gsz = {'f64': 8, 'f32': 4, 'bf16': 2}[dtype]
    assert prof[1] == 2 and prof[2] == 2.0 * nnz * (c_a + c_b), prof
    assert prof[3] == nnz * (2 * (4.0 + esz) + gsz * (c_a + c_b)), prof
    assert ws < 64 * (nnz + (n_a + n_b) * (c_a + c_b) * parts + (c_a + c_b) ** 2) + (6 << 20), ws      # never ~ n_a * n_b
    pw = ((n_b + parts - 1) // parts + 63) // 64 * 64
    ph = ((n_a + parts - 1) // parts + 63) // 64 * 64
    csc_order = np.lexsort((np.nonzero(pat)[0], np.nonzero(pat)[1]))
    c_ptr = np.zeros(n_b + 1, dtype=np.int64)
    np.cumsum(pat.sum(axis=0), out=c_ptr[1:])
    c_idx, c_val = np.nonzero(pat)[0][csc_order], ke.values[csc_order]
    if dtype in ('f64', 'f32'):
        Pm = model_pass(ke.indptr, ke.indices, ke.values, G0['b'], n_a, parts, pw, dtype)
        Qm = model_pass(c_ptr, c_idx, c_val, G0['a'], n_b, parts, ph, dtype)
        assert np.array_equal(P, Pm.astype(np.float64)), '%s: P = R G_j differs from the host model (max %.3e)' % (
            what, np.max(np.abs(P - Pm)))
        assert np.array_equal(Q, Qm.astype(np.float64)), '%s: Q = R^T G_i differs from the host model (max %.3e)' % (
            what, np.max(np.abs(Q - Qm)))
    else:
        u = K.U_ACC['bf16']
        for name, got, want, L in (('P = R G_j', P, R @ G0['b'], pat.sum(1)[:, None]),
                                   ('Q = R^T G_i', Q, R.T @ G0['a'], pat.sum(0)[:, None])):
            bound = (L + parts + 2) * u * want                  # (every term is positive: |R| |G| = R G)
            dev = np.abs(got - want)
            out[name] = np.max(np.where(dev == 0, 0.0, dev / np.maximum(K.K_SAFE * bound, 1e-300)))
            within(out[name], 1.0, '%s: valued lists over bf16 rows, %s, |delta| / model bound' % (what, name))
    # ---- the error pass: tr(S^T Gram_i S Gram_j) + sum over the stored entries of (r - x)^2 - x^2
    et = 'f32' if dtype == 'bf16' else dtype                   # (the error pass of the bf16 engine gathers the f32 masters)
    u = K.U_ACC[et]
    Hr, dH = K.gathered_T(Gi, S.T, et)                          # H = G_i S as the pass gathers it
    Gjr = K.store_round(Gj, et)
    x = Hr @ Gjr.T
    dx = (c_b + 2) * u * (np.abs(Hr) @ np.abs(Gjr).T) + dH @ np.abs(Gjr).T
    Kf = pat.astype(np.float64)
    X = Gi @ S @ Gj.T
    host = np.sum(X * X) + np.sum(Kf * ((R - x) ** 2 - x ** 2))
    bound = np.sum(Kf * (2 * (np.abs(R - x) + np.abs(x)) * dx + 4 * u * ((R - x) ** 2 + x ** 2)))
    bound += (n_a + n_b + 2 * (c_a + c_b)) * 2.0 ** -53 * np.sum((np.abs(Gi) @ np.abs(S) @ np.abs(Gj).T) ** 2)
    out['squared error'] = abs(sq - host) / (K.K_SAFE * bound)
    within(out['squared error'], 1.0, '%s: squared error (trace term + SRP_ERR pass), |delta| / model bound' % what)
    dense = np.sum((R - X) ** 2)                                # (and the formula itself: the dense statement in f64)
    assert abs(np.sum(X * X) + np.sum(Kf * ((R - X) ** 2 - X ** 2)) - dense) <= 1e-9 * dense
    return out


# ---- the lists a bind builds ------------------------------------------------------------------------------------------
def lists_case(n_a, n_b, c_a, c_b, dtype, parts, density, monkeypatch, seed=0, edits=()):
    """Row and column lists of a bound SKF_REL_SPARSE_CSR relation == scipy.sparse's tocsr() / tocsc() of the same matrix."""
    import scipy.sparse
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    rs = np.random.RandomState(seed)
    pat = rs.rand(n_a, n_b) < density
    if 'empty' in edits:
        pat[3, :] = False
        pat[:, 5] = False
    if 'full_row' in edits:
        pat[7, :] = True
    if 'none' in edits:
        pat[:] = False
    R = np.where(pat, eighths(rs, (n_a, n_b)) + (0.0 if dtype == 'bf16' else rs.rand(n_a, n_b)), 0.0)
    sp = scipy.sparse.coo_matrix((R[pat], np.nonzero(pat)), shape=R.shape)
    csr, csc = sp.tocsr(), sp.tocsc()
    csr.sort_indices()
    csc.sort_indices()
    ke = KnownEntries(csr.indptr, csr.indices, csr.data, csr.shape, unstored='zero')
    types, n, ranks = ['a', 'b'], {'a': n_a, 'b': n_b}, {'a': c_a, 'b': c_b}
    plan = DevicePlan(types, n, ranks, [('a', 'b', ke, None)], [], nat.SKF_DFMF, dtype=dtype)
    try:
        rp, ri, rv = plan.relation_lists(0, False)
        cp, ci, cv = plan.relation_lists(0, True)
    finally:
        plan.close()
    vt = np.float64 if dtype == 'f64' else np.float32
    assert np.array_equal(rp, csr.indptr) and np.array_equal(ri, csr.indices) and np.array_equal(rv, csr.data.astype(vt))
    assert np.array_equal(cp, csc.indptr) and np.array_equal(ci, csc.indices) and np.array_equal(cv, csc.data.astype(vt))


def invalid_lists_case(kind, dtype='f64', variant=None):
    """A broken CSR (or a missing hand-over) ends in SKF_E_INVALID at plan creation / bind, before any iteration."""
    rs = np.random.RandomState(5)
    n_a, n_b = 40, 30
    pat = rs.rand(n_a, n_b) < 0.2
    pat[0, :4] = True
    ke = stored_entries(np.where(pat, 1.0, 0.0), pat)
    if kind == 'indptr':
        ke.indptr[5], ke.indptr[6] = ke.indptr[6], ke.indptr[5] - 1
    elif kind == 'column':
        ke.indices[2] = n_b
    elif kind == 'order':
        ke.indices[0], ke.indices[1] = ke.indices[1], ke.indices[0]
    ke.validate = lambda: None                      # (the host check of the engine is not what is tested here)
    types, n, ranks = ['a', 'b'], {'a': n_a, 'b': n_b}, {'a': 8, 'b': 6}
    if kind == 'handover':
        import ctypes as C
        rt = nat.get_runtime()
        tdesc = (nat.TypeDesc * 2)()
        tdesc[0].n_obj, tdesc[0].rank, tdesc[1].n_obj, tdesc[1].rank = n_a, 8, n_b, 6
        rdesc = (nat.RelationDesc * 1)()
        rdesc[0].row_type, rdesc[0].col_type = 0, 1
        rdesc[0].flags, rdesc[0].known_bound = nat.SKF_REL_SPARSE_CSR, ke.known
        opt = nat.Options(nat.DTYPES[dtype], nat.SKF_DFMF, -1, nat.SKF_ENGINE_MFMA, 0, 0, 0)
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
        DevicePlan(types, n, ranks, [('a', 'b', ke, None)], [], nat.SKF_DFMF if variant is None else variant, dtype=dtype).close()
    assert exc.value.code == nat.SKF_E_INVALID


def invalid_flag_cases():
    """SKF_E_INVALID at plan creation: a fold-in plan, both CSR flags at once, a mask, a row block."""
    rt = nat.get_runtime()
    keep = rt.mem.empty(4096)

    def create(variant, flags, mask=False, n_rows=0, part_count=0, opt_flags=0):
        rel = dict(row_type=0, col_type=1, flags=flags, known_bound=10, n_rows=n_rows)
        if mask:
            rel.update(mask=keep.ptr, mask_ld=30)
        return plan_create_status(rt.lib, [(40, 8), (30, 6)], [rel], variant=variant, target=0 if variant == nat.SKF_TRANSFORM else -1,
                                  part=(0, part_count), opt_flags=opt_flags)[0]
    bad = -1                                            # SKF_E_INVALID
    assert nat.SKF_E_INVALID == bad
    assert create(nat.SKF_DFMF, nat.SKF_REL_SPARSE_CSR) == 0
    assert create(nat.SKF_DFMC, nat.SKF_REL_SPARSE_CSR) == 0
    assert create(nat.SKF_TRANSFORM, nat.SKF_REL_SPARSE_CSR) == bad
    assert create(nat.SKF_DFMC, nat.SKF_REL_SPARSE_CSR | nat.SKF_REL_KNOWN_CSR) == bad
    assert create(nat.SKF_DFMC, nat.SKF_REL_SPARSE_CSR, mask=True) == bad
    assert create(nat.SKF_DFMF, nat.SKF_REL_SPARSE_CSR, n_rows=20) == bad
    assert create(nat.SKF_DFMF, nat.SKF_REL_SPARSE_CSR, part_count=2) == bad
    assert create(nat.SKF_DFMF, nat.SKF_REL_SPARSE_CSR, part_count=2, opt_flags=nat.SKF_OPT_OWNED_ROWS) == bad


# ---- whole fits -------------------------------------------------------------------------------------------------------
def fusion_graph(n, ranks, seed=0, density=(0.02, 0.002), zero_rel=False, empty_side=False):
    """a-b and b-c sparse (stored values: multiples of 1/8 in (0, 8)), a-c dense, a sparse constraint on b."""
    rs = np.random.RandomState(seed)
    types = ['a', 'b', 'c']
    R_ab = np.where(rs.rand(n['a'], n['b']) < density[0], eighths(rs, (n['a'], n['b'])), 0.0)
    R_bc = np.where(rs.rand(n['b'], n['c']) < density[1], eighths(rs, (n['b'], n['c'])), 0.0)
    if zero_rel:
        R_bc[:] = 0.0                               # an all-zero relation: nnz = 0
    if empty_side:
        R_ab[: n['a'] // 2, :] = 0.0                # half of the row type's objects hold no entry, as do some columns
        R_ab[:, ::3] = 0.0
    R_ac = rs.rand(n['a'], n['c'])
    theta = -0.01 * (rs.rand(n['b'], n['b']) < 2.0 / n['b'])
    theta = theta + theta.T
    np.fill_diagonal(theta, 0.02)
    rels = [('a', 'b', R_ab), ('b', 'c', R_bc), ('a', 'c', R_ac)]
    G0 = {t: rs.rand(n[t], ranks[t]) + 0.1 for t in types}
    return types, rels, [('b', theta)], G0


def run_plan(types, n, ranks, rels, thetas, G0, dtype, iters, sparse, variant=None):
    """rels: (i, j, dense matrix); sparse: the indices of the relations handed over as their stored entries."""
    rl = [(i, j, stored_entries(R) if k in sparse else R, None) for k, (i, j, R) in enumerate(rels)]
    plan = DevicePlan(types, n, ranks, rl, thetas, nat.SKF_DFMF if variant is None else variant, dtype=dtype)
    try:
        for t in types:
            plan.set_factor(t, G0[t])
        errs = []
        for _ in range(iters):
            plan.iterate(1)
            errs.append([plan.relation_sqerr(k) for k in range(len(rels))])
        G = {t: plan.get_factor(t) for t in types}
        S = [plan.get_backbone(k) for k in range(len(rels))]
        return G, S, np.array(errs), plan.workspace_bytes
    finally:
        plan.close()


def csr_against_dense(n, ranks, dtype, tol, what, iters=4, seed=0, variant=None, **kw):
    """CSR-fed vs dense-fed plan of the same data and G0.  tol = (G, S, squared errors): the bounds the project holds its
    list path to against its dense path (tests/test_gpu_parity.py, sparse_against_dense)."""
    types, rels, thetas, G0 = fusion_graph(n, ranks, seed, **kw)
    Gs, Ss, Es, _ = run_plan(types, n, ranks, rels, thetas, G0, dtype, iters, (0, 1), variant)
    Gd, Sd, Ed, _ = run_plan(types, n, ranks, rels, thetas, G0, dtype, iters, (), variant)
    for t in types:
        assert np.isfinite(Gs[t]).all()
        within(relerr(Gs[t], Gd[t]), tol[0], '%s: CSR-fed vs dense-fed, G_%s after %d iterations' % (what, t, iters))
    for k in range(len(rels)):
        scale = max(np.linalg.norm(Sd[k]), 1e-300)
        within(np.linalg.norm(Ss[k] - Sd[k]) / scale, tol[1], '%s: CSR-fed vs dense-fed, S_%d' % (what, k))
    assert np.isfinite(Es).all()
    assert np.array_equal(Es[Ed == 0], Ed[Ed == 0])             # (an all-zero relation: S = 0, both errors exactly 0)
    within(np.max(np.where(Ed > 0, np.abs(Es - Ed) / np.where(Ed > 0, Ed, 1.0), 0.0)), tol[2],
           '%s: CSR-fed vs dense-fed, squared errors of every iteration' % what)
    return Es, Ed


def csr_against_oracle(n, ranks, iters, tol, what, seed=0, **kw):
    """f64 engine, CSR-fed, against oracle.dfmf_oracle.dfmf on the dense matrices: G, S and the per-relation errors."""
    from oracle import dfmf_oracle as orc
    types, rels, thetas, G0 = fusion_graph(n, ranks, seed, **kw)
    Gs, Ss, Es, _ = run_plan(types, n, ranks, rels, thetas, G0, 'f64', iters, (0, 1))
    R = {(i, j): [M] for i, j, M in rels}
    Theta = {(t, t): [M] for t, M in thetas}
    Go, So = orc.dfmf(R, Theta, types, ranks, max_iter=iters, G0={(t, t): G0[t] for t in types})
    for t in types:
        within(relerr(Gs[t], Go[t, t]), tol, '%s: CSR-fed f64 engine vs oracle, G_%s after %d iterations' % (what, t, iters))
    for k, (i, j, M) in enumerate(rels):
        within(relerr(Ss[k], So[i, j][0]), tol, '%s: CSR-fed f64 engine vs oracle, S_%d' % (what, k))
        want = np.sum((M - Go[i, i] @ So[i, j][0] @ Go[j, j].T) ** 2)
        within(abs(Es[-1][k] - want) / want, tol, '%s: CSR-fed f64 engine vs oracle, squared error of relation %d' % (what, k))


def refusal_order_case(which):
    """A stored-entry relation (SKF_REL_SPARSE_CSR) with defective lists: refused by the validation kernel alone."""
    import known_csr_cases as KC
    KC.refused_after_one_launch(lambda w: KC.small_plan(w, nat.SKF_DFMF, 'zero').close(), which)
