"""Relations with MISSING values fitted as entries plus rank one (SKF_REL_FILL_RANK1 on SKF_REL_SPARSE_CSR; csrc/skf_known.h:
colsum_partial_kernel, sum_parts_rank1_kernel; sparse_pass / fill_err_terms in csrc/skf_stages.inc) -- the SAME cases on the
host emulator (small) and on the GPU.  The filled matrix is F = a b^T + D, D sparse on the stored pattern with d = v - a_r b_c.

First part (no engine): Relation.filled_entries() against Relation.filled() of the MaskedArray form, the routing rule,
the initialisers.  Second part: one pass P = F G_j, one Q = F^T G_i and one error pass through DevicePlan, held to the host
(pass_case).  Third part: whole fits against the oracle on the expanded filled matrix, and the public API."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, KnownEntries
from skfusion_amd.fusion import FusionGraph, Relation, ObjectType, Dfmf, Dfmc
from skfusion_amd.fusion.decomposition import dfmf as dfmf_mod
from helpers import plan_create_status, relerr, within
import known_cases as K
import sparse_dfmf_cases as SC

FILLS = ('mean', 'row_mean', 'col_mean', 2.5)
COLSUM_ROWS = 128           # rows of a first-stage workgroup of the column-sum kernel (csrc/skf_known.h)
# f32 / bf16 fits against the f64 oracle on the filled matrix, (G, S, squared errors) after 10 iterations: about 5 x (never
# more than 10 x) the largest deviation measured on the MI355X over the four fills at N = 3000 / 2600 / 500, rank_b 64 / 128 /
# 256 (profiles/r17_filled_entries.txt: f32 3.8e-6 / 4.3e-5 / 4.1e-8, bf16 1.6e-2 / 7.8e-2 / 1.0e-4)
FIT_TOL = {'f32': (2e-5, 2e-4, 2e-7), 'bf16': (8e-2, 3.5e-1, 5e-4)}
# the public API, entries plus rank one against the dense expansion of the SAME engine (sparse_relations=False), (G, S) after
# 10 iterations at 900 x 700, ranks 128 / 64 / 32: measured f32 1.2e-5 / 1.7e-4, bf16 2.7e-3 / 1.5e-2 (same file); f64 holds
# the 1e-9 of the oracle comparison
API_TOL = {'f64': (1e-9, 1e-9), 'f32': (5e-5, 8e-4), 'bf16': (1.3e-2, 7e-2)}
# the host emulator at N = 150 / 130 / 40, ranks 20 / 24 / 5, fill 'row_mean' -- a site of its own (another size, so other
# relative deviations; its arithmetic is deterministic): measured f32 5.7e-7 / 9.5e-6 / 1.2e-7, bf16 3.0e-3 / 2.9e-2 / 5.8e-4
FIT_TOL_EMUL = {'f32': (3e-6, 5e-5, 6e-7), 'bf16': (1.5e-2, 1.5e-1, 3e-3)}


def fit_tol(dtype):
    """(G, S, squared errors): f64 the 1e-9 sparse_dfmf_cases.csr_against_oracle holds after 10 iterations."""
    return (1e-9, 1e-9, 1e-9) if dtype == 'f64' else FIT_TOL[dtype]


# ---- host: the container against Relation.filled() ----------------------------------------------------------------------
def dyadic_pattern(n_r, n_c, block=64, per_line=4, seed=0):
    """A stored pattern whose every mean is a short dyadic number: the leading block x block cells hold `per_line` entries
    in every row AND every column (a circulant), everything outside is not stored -- so rows and columns without an entry
    exist, nnz = block * per_line is a power of two, and with values that are multiples of 1/8 every sum the fills and the
    initialisers form is exact in f64, whatever its order."""
    assert block <= min(n_r, n_c) - 1
    rs = np.random.RandomState(seed)
    pat = np.zeros((n_r, n_c), dtype=bool)
    perm = rs.permutation(block)
    for s in range(per_line):
        pat[np.arange(block), perm[(np.arange(block) + 5 * s) % block]] = True
    assert (pat[:block].sum(1) == per_line).all() and (pat[:, :block].sum(0) == per_line).all()
    vals = np.where(pat, rs.randint(1, 64, size=pat.shape) / 8.0, 0.0)
    return pat, vals


def sparse_of(pat, vals):
    return scipy.sparse.csr_matrix(scipy.sparse.coo_matrix((vals[pat], np.nonzero(pat)), shape=pat.shape))


def masked_of(pat, vals):
    return np.ma.MaskedArray(np.where(pat, vals, 0.0), mask=~pat)


def two_types(ranks=(6, 5)):
    return ObjectType('rows', ranks[0]), ObjectType('cols', ranks[1])


def container_case(fill, n=(90, 75)):
    """filled_entries().expand() == Relation(MaskedArray form).filled(), data and mask, bit for bit."""
    pat, vals = dyadic_pattern(*n)
    tr, tc = two_types()
    ke = Relation(sparse_of(pat, vals), tr, tc, fill_value=fill, unstored='unknown').filled_entries()
    want = Relation(masked_of(pat, vals), tr, tc, fill_value=fill).filled()
    assert ke.unstored == 'zero' and ke.known == int(pat.sum())
    assert np.array_equal(ke.expand(), np.ma.getdata(want))
    # the mask: 'mean' and numbers keep it (the entries not stored), the line means leave every entry known
    stored = np.zeros(pat.shape, dtype=bool)
    stored[ke.rows_cols()] = True
    got_mask = ~stored if (fill == 'mean' or not isinstance(fill, str)) else np.zeros(pat.shape, dtype=bool)
    assert np.array_equal(got_mask, np.ma.getmaskarray(want))
    assert (ke.row_fill == 1.0).all() or (ke.col_fill == 1.0).all()
    # rows / columns without an entry take the overall mean m = data.sum() / nnz
    m = vals[pat].sum() / pat.sum()
    if fill == 'row_mean':
        assert (ke.row_fill[pat.sum(1) == 0] == m).all() and (pat.sum(1) == 0).any()
    if fill == 'col_mean':
        assert (ke.col_fill[pat.sum(0) == 0] == m).all() and (pat.sum(0) == 0).any()


def routing_case():
    """What filled_entries_apply takes and what it leaves to the dense expansion."""
    pat, vals = dyadic_pattern(90, 75)
    tr, tc = two_types()
    sp = sparse_of(pat, vals)
    app = dfmf_mod.filled_entries_apply
    for fill in FILLS:
        rel = Relation(sp, tr, tc, fill_value=fill, unstored='unknown')
        assert app(rel, True)
        assert app(rel, True, 'runs', 'dfmc') == (fill in ('row_mean', 'col_mean'))
        assert not app(rel, False) and not app(rel, None)           # (None: a small graph stays on its schedule)
        for shard in ('owned', 'rows', 'relations'):
            assert not app(rel, True, shard)
    big = (ObjectType('rows', 70), tc)                               # a rank above 64: beyond the small-graph limits
    assert app(Relation(sp, big[0], big[1], unstored='unknown'), None)
    dense = sparse_of(np.ones_like(pat), vals + 1.0)
    assert not app(Relation(dense, tr, tc, unstored='unknown'), True)                      # every entry stored
    nan = sp.copy()
    nan.data[3] = np.nan
    assert not app(Relation(nan, tr, tc, unstored='unknown'), True)                        # a stored NaN
    assert not app(Relation(sp, tr, tc, unstored='unknown', preprocessor=lambda x: x), True)
    assert not app(Relation(sp, tr, tc), True)                                             # unstored='zero': the other path
    assert not app(Relation(sparse_of(pat[:75, :75], vals[:75, :75]), tr, tr, unstored='unknown'), True)
    # graph_matrices routes: Dfmf all four, Dfmc the line means (the others to its known-entry lists)
    for fill in FILLS:
        g = FusionGraph([Relation(sp, tr, tc, fill_value=fill, unstored='unknown')])
        R, _ = dfmf_mod.graph_matrices(g, sparse_relations=True)
        assert isinstance(R[tr, tc][0], KnownEntries) and R[tr, tc][0].row_fill is not None
        R, _, M = dfmf_mod.graph_matrices(g, with_masks=True, known_entries=True, sparse_relations=True, variant='dfmc')
        assert isinstance(R[tr, tc][0], KnownEntries) and M[tr, tc][0] is None
        assert (R[tr, tc][0].row_fill is not None) == (fill in ('row_mean', 'col_mean'))
        R, _ = dfmf_mod.graph_matrices(g, sparse_relations=False)
        assert isinstance(R[tr, tc][0], np.ndarray)


def initialiser_case(init_type, fill, seed=2):
    """G0 from the entries view == G0 from the expanded filled matrix, and the RandomState is consumed alike.  (The sums
    are exact by construction -- dyadic_pattern --, so their order does not show.)"""
    pat, vals = dyadic_pattern(90, 75)
    tr, tc = two_types()
    ke = Relation(sparse_of(pat, vals), tr, tc, fill_value=fill, unstored='unknown').filled_entries()
    out = []
    for R in ({(tr, tc): [ke]}, {(tr, tc): [ke.expand()]}):
        rs = np.random.RandomState(seed)
        G0 = dfmf_mod.initial_factors(R, [tr, tc], {tr: 6, tc: 5}, init_type, rs, 2)
        out.append((G0, rs.rand(3)))
    for ga, gb in zip(out[0][0], out[1][0]):
        for key in ga:
            assert np.array_equal(ga[key], gb[key]), 'G0 of %s (%s, fill %r) differs from the filled matrix\'s' % (key[0], init_type, fill)
    assert np.array_equal(out[0][1], out[1][1])


# ---- one pass through DevicePlan ------------------------------------------------------------------------------------------
def fill_vector(rs, n):
    """Multiples of 1/8 in (0, 8), not constant."""
    v = rs.randint(1, 64, size=n) / 8.0
    v[0], v[-1] = 0.125, 7.875
    return v


def filled_container(pat, vals, a, b):
    ke = SC.stored_entries(np.where(pat, vals, 0.0), pat)
    return KnownEntries(ke.indptr, ke.indices, ke.values, ke.shape, unstored='zero', row_fill=a, col_fill=b)


def pass_case(n_a, n_b, c_a, c_b, dtype, parts, pattern, what, monkeypatch, seed=0, lengths=K.LIST_LENGTHS):
    """One a x b relation F = a b^T + D with a general a AND b (multiples of 1/8 in (0, 8), neither constant: a swap of the
    two shows), stored values multiples of 1/8, so d = v - a_r b_c is a multiple of 1/64 below 64: exact in every type.
    DFMF on the engine `dtype`, lists in `parts` parts.
      lists    relation_lists values == d, np.array_equal.
      P, Q     of the first iteration (from a low-bit G0) against sparse_dfmf_cases.model_pass(d) + a t^T, t = G_j^T b
               (s = G_i^T a for Q) -- t, s exact in f64 and in f32 (multiples of 2^-11 below 2^12).
               f64: every product and sum is exact: np.array_equal.
               f32: the list part's order is the model's; then one product a_r t_q and one add, each rounded once:
                    |delta| <= 2 u (|model| + |a t^T|), u = 2^-24.
               bf16: the bound of sparse_dfmf_cases.pass_case with |D| |G| in place of R G (d has both signs),
                    K_SAFE (L + parts + 2) u |D| |G|, plus the same 2 u (|want| + |a t^T|).
      error    against the host's tr(S^T Gram_i S Gram_j) + |a|^2 |b|^2 - 2 (a^T G_i) S (G_j^T b)
               + sum over the stored of (d - x)^2 - x^2 + 2 sum d a b, with the bound of sparse_dfmf_cases.pass_case (d for
               r) extended by the f64 rounding of the three new terms: sums of n terms in f64 carry at most (n + 1) 2^-53
               of the sum of the magnitudes, so
                   |a|^2 |b|^2:              (n_a + n_b + 1) 2^-53 |a|^2 |b|^2
                   2 sum d a b:              (nnz + 3) 2^-53 2 sum |d a b|
                   2 (a^T G_i) S (G_j^T b):  (n_a + n_b + c_a c_b + 4) 2^-53 2 (|a|^T |G_i|) |S| (|G_j|^T |b|)
               and the three additions into the trace term's slot, 3 x 2^-53 of the sum of the four magnitudes; times
               K_SAFE like every other first-order bound here.  (G_i, G_j are the masters in every engine and S is f64, so the
               host multiplies the operands the device multiplies.)"""
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    rs = np.random.RandomState(seed)
    pat = K.edge_mask(n_a, n_b, pattern, seed, lengths)
    vals = SC.eighths(rs, (n_a, n_b))
    a, b = fill_vector(rs, n_a), fill_vector(rs, n_b)
    ke = filled_container(pat, vals, a, b)
    rows, cols = np.nonzero(pat)
    d = vals[rows, cols] - a[rows] * b[cols]                    # exact
    D = np.zeros((n_a, n_b))
    D[rows, cols] = d
    bits = 6 if dtype == 'bf16' else 8
    G0 = {'a': SC.low_bit_factor(rs, n_a, c_a, bits), 'b': SC.low_bit_factor(rs, n_b, c_b, bits)}
    types, n, ranks = ['a', 'b'], {'a': n_a, 'b': n_b}, {'a': c_a, 'b': c_b}
    plan = DevicePlan(types, n, ranks, [('a', 'b', ke, None)], [], nat.SKF_DFMF, dtype=dtype)
    try:
        rp, ri, rv = plan.relation_lists(0, False)
        cp, ci, cv = plan.relation_lists(0, True)
        for t in types:
            plan.set_factor(t, G0[t])
        plan.set_profiling(True)
        plan.iterate(1)
        prof = plan.get_profile()
        plan.set_profiling(False)
        P = plan.get_contraction(0, 0).astype(np.float64)
        Q = plan.get_contraction(0, 1).astype(np.float64)
        S = plan.get_backbone(0).astype(np.float64)
        Gi, Gj = plan.get_factor('a').astype(np.float64), plan.get_factor('b').astype(np.float64)
        sq = plan.relation_sqerr(0)
        ws = plan.workspace_bytes
    finally:
        plan.close()
    nnz = int(pat.sum())
    vt = np.float64 if dtype == 'f64' else np.float32
    csc_order = np.lexsort((rows, cols))
    assert np.array_equal(ri, cols) and np.array_equal(rv, d.astype(vt)), '%s: the row lists do not hold v - a_r b_c' % what
    assert np.array_equal(ci, rows[csc_order]) and np.array_equal(cv, d[csc_order].astype(vt)), '%s: column lists' % what
    # the profile: the two list passes as before, one more counted launch each for the rank-one side (include/skfusion_hip.h)
    esz = {'f64': 8, 'f32': 4, 'bf16': 4}[dtype]
    gsz = {'f64': 8, 'f32': 4, 'bf16': 2}[dtype]
    extra_bytes = (n_b * (c_b * gsz + esz) + n_a * esz) + (n_a * (c_a * gsz + esz) + n_b * esz)
    if parts == 1:
        extra_bytes += 2 * esz * (n_a * c_b + n_b * c_a)
    assert prof[1] == 4, prof
    assert prof[2] == 2.0 * nnz * (c_a + c_b) + 2.0 * (n_b * c_b + n_a * c_b) + 2.0 * (n_a * c_a + n_b * c_a), prof
    assert prof[3] == nnz * (2 * (4.0 + esz) + gsz * (c_a + c_b)) + extra_bytes, prof
    # the bound sparse_dfmf_cases.pass_case asserts, plus 64 (n_i + n_j): never ~ n_a * n_b
    assert ws < 64 * (nnz + (n_a + n_b) * (c_a + c_b) * parts + (c_a + c_b) ** 2) + (6 << 20) + 64 * (n_a + n_b), ws
    pw = ((n_b + parts - 1) // parts + 63) // 64 * 64
    ph = ((n_a + parts - 1) // parts + 63) // 64 * 64
    c_ptr = np.zeros(n_b + 1, dtype=np.int64)
    np.cumsum(pat.sum(axis=0), out=c_ptr[1:])
    c_idx, c_val = rows[csc_order], d[csc_order]
    t, s = G0['b'].T @ b, G0['a'].T @ a                          # exact
    out = {}
    sides = (('P = F G_j', P, (ke.indptr, ke.indices, d, G0['b'], n_a, parts, pw), np.outer(a, t), D @ G0['b'],
              np.abs(D) @ G0['b'], pat.sum(1)[:, None]),
             ('Q = F^T G_i', Q, (c_ptr, c_idx, c_val, G0['a'], n_b, parts, ph), np.outer(b, s), D.T @ G0['a'],
              np.abs(D).T @ G0['a'], pat.sum(0)[:, None]))
    for name, got, margs, r1, lists_exact, lists_abs, L in sides:
        if dtype == 'f64':
            model = SC.model_pass(*margs, dtype=dtype).astype(np.float64) + r1
            assert np.array_equal(got, model), '%s: %s differs from model_pass(d) + a t^T (max %.3e)' % (
                what, name, np.max(np.abs(got - model)))
            continue
        u = 2.0 ** -24
        if dtype == 'f32':
            model = SC.model_pass(*margs, dtype=dtype).astype(np.float64)
            bound = 2 * u * (np.abs(model) + np.abs(r1))
            dev = np.abs(got - (model + r1))
        else:
            bound = K.K_SAFE * (L + parts + 2) * u * lists_abs + 2 * u * (np.abs(lists_exact + r1) + np.abs(r1))
            dev = np.abs(got - (lists_exact + r1))
        out[name] = np.max(np.where(dev == 0, 0.0, dev / np.maximum(bound, 1e-300)))
        within(out[name], 1.0, '%s: %s, |delta| / bound' % (what, name))
    # ---- the error pass
    et = 'f32' if dtype == 'bf16' else dtype
    u = K.U_ACC[et]
    Hr, dH = K.gathered_T(Gi, S.T, et)
    Gjr = K.store_round(Gj, et)
    x = Hr @ Gjr.T
    dx = (c_b + 2) * u * (np.abs(Hr) @ np.abs(Gjr).T) + dH @ np.abs(Gjr).T
    Kf = pat.astype(np.float64)
    X = Gi @ S @ Gj.T
    ab = np.outer(a, b)
    t_trace, t_const = np.sum(X * X), np.sum(a * a) * np.sum(b * b)
    t_usv, t_dab = 2.0 * ((a @ Gi) @ S @ (Gj.T @ b)), 2.0 * np.sum(Kf * D * ab)
    host = t_trace + t_const - t_usv + np.sum(Kf * ((D - x) ** 2 - x ** 2)) + t_dab
    bound = np.sum(Kf * (2 * (np.abs(D - x) + np.abs(x)) * dx + 4 * u * ((D - x) ** 2 + x ** 2)))
    bound += (n_a + n_b + 2 * (c_a + c_b)) * 2.0 ** -53 * np.sum((np.abs(Gi) @ np.abs(S) @ np.abs(Gj).T) ** 2)
    e53 = 2.0 ** -53
    bound += (n_a + n_b + 1) * e53 * t_const
    bound += (nnz + 3) * e53 * 2.0 * np.sum(Kf * np.abs(D) * ab)
    usv_abs = 2.0 * ((a @ np.abs(Gi)) @ np.abs(S) @ (np.abs(Gj).T @ b))
    bound += (n_a + n_b + c_a * c_b + 4) * e53 * usv_abs
    bound += 3 * e53 * (abs(t_trace) + t_const + usv_abs + abs(t_dab))
    out['squared error'] = abs(sq - host) / (K.K_SAFE * bound)
    within(out['squared error'], 1.0, '%s: squared error of the filled relation, |delta| / model bound' % what)
    F = ab + D                                                  # (and the formula itself: the dense statement in f64)
    dense = np.sum((F - X) ** 2)
    formula = t_trace + t_const - t_usv + np.sum(Kf * ((D - X) ** 2 - X ** 2)) + t_dab
    assert abs(formula - dense) <= 1e-9 * dense
    return out


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _raw_create(variant, flags, opt_flags=0, part_count=0):
    return plan_create_status(nat.get_runtime().lib, [(40, 8), (30, 6)], [dict(row_type=0, col_type=1, flags=flags, known_bound=10)],
                              variant=variant, target=0 if variant == nat.SKF_TRANSFORM else -1, part=(0, part_count), opt_flags=opt_flags)[0]


def refused_flag_cases():
    """SKF_E_INVALID at plan creation: the flag on an owned plan, on a transform plan, without SKF_REL_SPARSE_CSR."""
    both = nat.SKF_REL_SPARSE_CSR | nat.SKF_REL_FILL_RANK1
    assert _raw_create(nat.SKF_DFMF, both) == 0
    assert _raw_create(nat.SKF_DFMC, both) == 0
    assert _raw_create(nat.SKF_DFMF, nat.SKF_REL_FILL_RANK1) == nat.SKF_E_INVALID
    assert _raw_create(nat.SKF_DFMC, nat.SKF_REL_FILL_RANK1 | nat.SKF_REL_KNOWN_CSR) == nat.SKF_E_INVALID
    assert _raw_create(nat.SKF_TRANSFORM, both) == nat.SKF_E_INVALID
    assert _raw_create(nat.SKF_TRANSFORM, nat.SKF_REL_FILL_RANK1 | nat.SKF_REL_FOLD_CSR) == nat.SKF_E_INVALID
    assert _raw_create(nat.SKF_DFMF, both | nat.SKF_REL_ABSENT, nat.SKF_OPT_OWNED_ROWS, 2) == nat.SKF_E_INVALID
    assert _raw_create(nat.SKF_DFMF, both, nat.SKF_OPT_OWNED_ROWS, 1) == nat.SKF_E_INVALID


def refused_at_bind_case(kind, dtype='f64'):
    """The flag without skf_plan_set_relation_fill, and a NaN in a: SKF_E_INVALID at bind, before anything gathers."""
    rs = np.random.RandomState(5)
    n_a, n_b = 40, 30
    pat = rs.rand(n_a, n_b) < 0.2
    a, b = fill_vector(rs, n_a), fill_vector(rs, n_b)
    ke = filled_container(pat, SC.eighths(rs, (n_a, n_b)), a, b)
    types, n, ranks = ['a', 'b'], {'a': n_a, 'b': n_b}, {'a': 8, 'b': 6}
    if kind == 'nan':
        ke.row_fill[7] = np.nan
        ke.validate = lambda: None                      # (the host check of the engine is not what is tested here)
        from skfusion_amd._engine import launch_count
        before = launch_count()
        with pytest.raises(nat.SkfNativeError) as exc:
            DevicePlan(types, n, ranks, [('a', 'b', ke, None)], [], nat.SKF_DFMF, dtype=dtype).close()
        assert exc.value.code == nat.SKF_E_INVALID
        assert launch_count() - before == 2             # the validation -- the lists, then the two vectors --, nothing after it
        return
    assert kind == 'missing'
    rt = nat.get_runtime()
    from skfusion_amd._engine import upload_known_entries
    dev = upload_known_entries(ke, dtype, rt.mem)
    tdesc = (nat.TypeDesc * 2)()
    tdesc[0].n_obj, tdesc[0].rank, tdesc[1].n_obj, tdesc[1].rank = n_a, 8, n_b, 6
    rdesc = (nat.RelationDesc * 1)()
    rdesc[0].row_type, rdesc[0].col_type = 0, 1
    rdesc[0].flags, rdesc[0].known_bound = nat.SKF_REL_SPARSE_CSR | nat.SKF_REL_FILL_RANK1, ke.known
    opt = nat.Options(nat.DTYPES[dtype], nat.SKF_DFMF, -1, nat.SKF_ENGINE_MFMA, 0, 0, 0)
    handle = nat._P()
    rt.call('skf_plan_create', 2, tdesc, 1, rdesc, 0, (nat.ThetaDesc * 1)(), C.byref(opt), C.byref(handle))
    try:
        rt.call('skf_plan_set_known_entries', handle, 0, dev.indptr.ptr, dev.indices.ptr, dev.values.ptr)
        nbytes = C.c_size_t()
        rt.call('skf_plan_workspace_bytes', handle, C.byref(nbytes))
        ws = rt.mem.empty(nbytes.value)
        with pytest.raises(nat.SkfNativeError) as exc:
            rt.call('skf_plan_bind_workspace', handle, ws.ptr, nbytes.value, rt.mem.stream)
        assert exc.value.code == nat.SKF_E_INVALID
    finally:
        rt.lib.skf_plan_destroy(handle)
    # ... and the entry point itself refuses a relation without the flag
    rdesc[0].flags = nat.SKF_REL_SPARSE_CSR
    handle = nat._P()
    rt.call('skf_plan_create', 2, tdesc, 1, rdesc, 0, (nat.ThetaDesc * 1)(), C.byref(opt), C.byref(handle))
    try:
        assert rt.lib.skf_plan_set_relation_fill(handle, 0, dev.row_fill.ptr, dev.col_fill.ptr, None) == nat.SKF_E_INVALID
    finally:
        rt.lib.skf_plan_destroy(handle)


# ---- whole fits -------------------------------------------------------------------------------------------------------------
def fit_graph(n, ranks, fill, seed=0, density=0.02):
    """a-b with missing values (stored values: multiples of 1/8 in (0, 8); an empty row and an empty column) filled by
    `fill`, b-c sparse with zeros elsewhere, a-c dense, a sparse constraint on b -- sparse_dfmf_cases.fusion_graph with its
    first relation a ratings matrix.  Returns the types, the relations as (i, j, what the plan takes, the dense matrix the
    oracle takes), the constraints and G0."""
    types, rels, thetas, G0 = SC.fusion_graph(n, ranks, seed, density=(density, 0.002))
    rs = np.random.RandomState(seed + 100)
    pat = rs.rand(n['a'], n['b']) < density
    pat[3, :] = False
    pat[:, 5] = False
    vals = SC.eighths(rs, pat.shape)
    ta, tb = ObjectType('a', ranks['a']), ObjectType('b', ranks['b'])
    ke = Relation(sparse_of(pat, vals), ta, tb, fill_value=fill, unstored='unknown').filled_entries()
    full = np.ma.getdata(Relation(masked_of(pat, vals), ta, tb, fill_value=fill).filled())
    out = [('a', 'b', ke, full), ('b', 'c', SC.stored_entries(rels[1][2]), rels[1][2]), ('a', 'c', rels[2][2], rels[2][2])]
    return types, out, thetas, G0


def run_fit(types, n, ranks, rels, thetas, G0, dtype, iters, variant=nat.SKF_DFMF, dense=False):
    rl = [(i, j, full if dense else data, None) for i, j, data, full in rels]
    plan = DevicePlan(types, n, ranks, rl, thetas, variant, dtype=dtype)
    try:
        for t in types:
            plan.set_factor(t, G0[t])
        plan.iterate(iters)
        G = {t: plan.get_factor(t).astype(np.float64) for t in types}
        S = [plan.get_backbone(k).astype(np.float64) for k in range(len(rels))]
        E = np.array([plan.relation_sqerr(k) for k in range(len(rels))])
        return G, S, E
    finally:
        plan.close()


def fit_deviations(n, ranks, fill, dtype, iters=10, variant=nat.SKF_DFMF, seed=0):
    """The entries-fed fit against the f64 oracle on the expanded filled matrix: worst relative deviation of G, of S and of
    the per-relation squared errors after `iters` iterations."""
    from oracle import dfmf_oracle as orc
    types, rels, thetas, G0 = fit_graph(n, ranks, fill, seed)
    G, S, E = run_fit(types, n, ranks, rels, thetas, G0, dtype, iters, variant)
    R = {(i, j): [full] for i, j, _, full in rels}
    Theta = {(t, t): [M] for t, M in thetas}
    kw = dict(max_iter=iters, G0={(t, t): G0[t] for t in types})
    if variant == nat.SKF_DFMC:
        Go, So = orc.dfmc(R, {k: [None] for k in R}, Theta, types, ranks, **kw)
    else:
        Go, So = orc.dfmf(R, Theta, types, ranks, **kw)
    for t in types:
        assert np.isfinite(G[t]).all()
    dev_g = max(relerr(G[t], Go[t, t]) for t in types)
    dev_s = max(relerr(S[k], So[i, j][0]) for k, (i, j, _, _) in enumerate(rels))
    want = np.array([np.sum((full - Go[i, i] @ So[i, j][0] @ Go[j, j].T) ** 2) for i, j, _, full in rels])
    dev_e = float(np.max(np.abs(E - want) / want))
    return dev_g, dev_s, dev_e


def fit_against_oracle(n, ranks, fill, dtype, tol, what, **kw):
    """tol = (G, S, squared errors)."""
    dev = fit_deviations(n, ranks, fill, dtype, **kw)
    print('%s: deviation from the f64 oracle: G %.3e  S %.3e  squared errors %.3e' % ((what,) + dev))
    for v, t, name in zip(dev, tol, ('G', 'S', 'squared errors')):
        within(v, t, '%s: entries plus rank one vs oracle on the filled matrix, %s' % (what, name))
    return dev


def dfmc_repeat_case(n, ranks, dtype='f64'):
    """Two runs of the same DFMC fit give the same bits (no atomics anywhere on the rank-one side)."""
    types, rels, thetas, G0 = fit_graph(n, ranks, 'row_mean', 1)
    a = run_fit(types, n, ranks, rels, thetas, G0, dtype, 3, nat.SKF_DFMC)
    b = run_fit(types, n, ranks, rels, thetas, G0, dtype, 3, nat.SKF_DFMC)
    for t in types:
        assert np.array_equal(a[0][t], b[0][t])
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y)
    assert np.array_equal(a[2], b[2])


# ---- the public API -------------------------------------------------------------------------------------------------------
def ratings(n_u, n_m, density, seed):
    """A ratings-like scipy CSR (values multiples of 1/8) with an empty row and an empty column."""
    rs = np.random.RandomState(seed)
    pat = rs.rand(n_u, n_m) < density
    pat[2, :] = False
    pat[:, 4] = False
    return sparse_of(pat, rs.randint(1, 41, size=pat.shape) / 8.0)


def api_graph(sp, fill, ranks=(16, 12, 4), n_g=12, seed=1):
    rs = np.random.RandomState(seed)
    users, movies, genres = ObjectType('users', ranks[0]), ObjectType('movies', ranks[1]), ObjectType('genres', ranks[2])
    return FusionGraph([Relation(sp, users, movies, name='ratings', fill_value=fill, unstored='unknown'),
                        Relation((rs.rand(sp.shape[1], n_g) < 0.3).astype(float), movies, genres, name='genres')])


def forbid_expansion(monkeypatch, sp):
    """sparse_dfmf_api_cases.forbid_toarray, and the two methods of Relation that expand an unstored='unknown' relation."""
    import sparse_dfmf_api_cases as AC

    def guard(original):
        def method(self, *a, **k):
            if self.is_known_entries():
                raise AssertionError('a relation with missing values was expanded')
            return original(self, *a, **k)
        return method
    for name in ('dense_data', 'filled', 'filled_device'):
        monkeypatch.setattr(Relation, name, guard(getattr(Relation, name)))
    return AC.forbid_toarray(monkeypatch, sp)


def api_case(cls, fill, dtype, n, monkeypatch, ranks=(16, 12, 4), n_g=12, max_iter=10):
    """Dfmf / Dfmc(sparse_relations=True).fuse on an unstored='unknown' relation with expansion forbidden; the same fit
    with sparse_relations=False (the dense expansion) agrees within API_TOL (G, S)."""
    tol = API_TOL[dtype]
    import sparse_dfmf_api_cases as AC
    sp = ratings(n[0], n[1], 0.03, 3)
    args = dict(max_iter=max_iter, init_type='random', random_state=0, dtype=dtype)
    gd = api_graph(sp, fill, ranks, n_g)
    b = cls(sparse_relations=False, **args).fuse(gd)                # (first: nothing is forbidden yet)
    with monkeypatch.context() as mp:
        gs = api_graph(forbid_expansion(mp, sp.copy()), fill, ranks, n_g)
        a = cls(sparse_relations=True, **args).fuse(gs)
    AC.same_fit(a, b, gs, gd, False, tol, '%s %s fill %r' % (cls.__name__, dtype, fill))
    return a, gs


def api_everything_else_case(n, dtype, tmp_path, monkeypatch):
    """compute_err / stopping (the rule ends both fits at the same iteration, within the ten iterations the whole-fit bounds
    are stated for), n_run=3, complete() and save / load on a fit through entries plus rank one."""
    import sparse_dfmf_api_cases as AC
    from skfusion_amd.fusion.base import load_fit
    sp = ratings(n[0], n[1], 0.03, 7)
    seen = {True: [], False: []}
    fits = {}
    for sparse in (True, False):
        g = api_graph(sp, 'row_mean')
        rel = [r for r in g.relations if r.name == 'ratings'][0]
        # (the threshold follows the norm of the relation, ~ sqrt(cells); init 'random': both fits start from the same bits.  The column-mean initialisers sum the fill in another order
        # on the entries view, and their nearly collinear G0 makes S answer a last-bit change of G0 with 1e-8.)
        f = Dfmf(max_iter=10, init_type='random', random_state=3, dtype=dtype, compute_err=True, sparse_relations=sparse,
                 stopping=((rel.row_type, rel.col_type), 9e-4 * np.sqrt(n[0] * n[1])), callback=lambda G, S, it, k=sparse: seen[k].append(it))
        fits[sparse] = (f.fuse(g), g)
    print('iterations before the stopping rule ended the fits:', seen)
    assert seen[True] == seen[False] and 2 < len(seen[True]) < 10, (seen[True], seen[False])
    AC.same_fit(fits[True][0], fits[False][0], fits[True][1], fits[False][1], False, API_TOL[dtype], 'stopping')
    kw = dict(max_iter=3, init_type='random', random_state=5, dtype=dtype, n_run=3, sparse_relations=True)
    ga, gb = api_graph(sp, 'mean'), api_graph(sp, 'mean')
    AC.same_fit(Dfmf(n_jobs=3, **kw).fuse(ga), Dfmf(n_jobs=1, **kw).fuse(gb), ga, gb, True, what='n_run=3, n_jobs=3 vs 1')
    g = api_graph(sp, 'col_mean')
    f = Dfmf(max_iter=3, init_type='random_vcol', random_state=2, dtype=dtype, sparse_relations=True).fuse(g)
    rel = [r for r in g.relations if r.name == 'ratings'][0]
    full = f.complete(rel)
    assert full.shape == sp.shape and np.isfinite(full).all()
    assert np.allclose(full, f.factor(rel.row_type) @ f.backbone(rel) @ f.factor(rel.col_type).T)
    loaded = load_fit(f.save(str(tmp_path / 'fit.npz')), g)
    assert np.array_equal(loaded.complete(rel), full)
