"""Ownership-sharded fits (SKF_OPT_OWNED_ROWS, `shard='owned'`) whose relations are handed over as CSR and never densified:
every rank gives its plan the CSR of its OWNED rows over all columns (SKF_REL_SPARSE_CSR: unstored = zero; SKF_REL_KNOWN_CSR:
unstored = unknown), a rank without rows of the row type marks the relation absent -- the SAME cases on the host emulator
and on the GPU.  Ranks are threads of this process on one device (helpers.fit_owned / helpers.ThreadGroup).

Bounds.  f64 against the oracle: 1e-9 on G and S (what test_owned_sharding.py holds owned fits to), 1e-8 relative on the
summed squared errors.  CSR-fed owned fit against DENSE-fed owned fit (the latter is code from before this hand-over
existed): the project's list-versus-dense bounds, TOL of test_gpu_sparse_dfmf.py for the stored-entry relations and the
forced-list bounds of test_gpu_known_csr.py for the known-entry ones; there the dense-fed fit keeps the lists of its mask
(SKF_DFMC_SPARSE=1), the same lists byte for byte, so that comparison is also held to np.array_equal, as
known_csr_cases.csr_against_mask holds the single-device plans."""
import ctypes as C

import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, DeviceKnownEntries, KnownEntries, owned_rows
from skfusion_amd._engine import flatten_relations, flatten_thetas, count_objects
from skfusion_amd.fusion.decomposition._dfmf import owned_plan, _host_loop
from helpers import plan_create_status, relerr, within, fit_owned, ThreadGroup

import known_cases as K
import known_csr_cases as KC
import sparse_dfmf_cases as SC

N_LISTS = {'a': 459, 'b': 453, 'c': 130}        # 8 parts of 64 with tails of 11 and 5 (test_gpu_sparse_dfmf.py)
N_FIT = {'a': 200, 'b': 140, 'c': 130}          # bf16: the ownership chunk is 64-aligned, rank 2 of 3 owns no row of 'a'

# list path against dense path: (G, S, squared error)
TOL_SP0 = {'f64': (1.5e-12, 6e-12, 1.3e-13), 'f32': (7e-6, 3.5e-5, 1.5e-7), 'bf16': (1.2e-2, 2.5e-2, 5.5e-4)}
# DFMC, known-entry lists (test_gpu_known_csr.py, forced lists against the dense completion); bf16: that module states
# bit-identity with the mask form's lists only, which is asserted besides -- the bf16 list-versus-dense bound stands in
TOL_KNOWN = {'f64': (5e-12, 1.2e-11, 3e-13), 'f32': (7e-6, 3.5e-5, 1.5e-7), 'bf16': (1.2e-2, 2.5e-2, 5.5e-4)}

# The same comparison on ONE device (sparse_dfmf_cases.csr_against_dense, N_FIT, density (0.05, 0.03), worst of
# SKF_KNOWN_PARTS 1 / 4 and of the host emulator / the MI355X) measured on the commit before this hand-over existed, where
# the owned comparison exceeds TOL_SP0 because N_FIT is smaller than the shapes TOL_SP0 was measured at: the bound is then
# 10 x the single-device figure, the project's rule.  Every other component of every rank set keeps TOL_SP0.
#   f64 ranks 70 / 128 / 33, S: owned 7.5e-12 against 6e-12; single device 1.04e-11 -> 1.04e-10
#   bf16 ranks 256 / 128 / 64, squared error: owned 4.5e-3 against 5.5e-4; single device 4.77e-3 -> 4.77e-2
# (profiles/r15_sparse_owned.txt holds every figure.)
SHAPE_TOL = {('f64-wide', 1): 10 * 1.04e-11, ('bf16-256', 2): 10 * 4.77e-3}


def sp0_tol(key):
    return tuple(SHAPE_TOL.get((key, q), t) for q, t in enumerate(TOL_SP0[RANKS[key][0]]))


# ranks on both sides of the list kernels' width classes
RANKS = {'f64-narrow': ('f64', {'a': 16, 'b': 12, 'c': 8}), 'f64-wide': ('f64', {'a': 70, 'b': 128, 'c': 33}),
         'f32': ('f32', {'a': 64, 'b': 256, 'c': 24}),
         'bf16-128': ('bf16', {'a': 128, 'b': 64, 'c': 16}), 'bf16-256': ('bf16', {'a': 256, 'b': 128, 'c': 64})}


# ---- 1. creation: the status of skf_plan_create alone ------------------------------------------------------------------
def creation_cases():
    """Accepted on an owned plan: a CSR-fed relation whose block is the owned range, and one flagged SKF_REL_ABSENT where
    the rank owns no row.  Refused: a block that is not the owned range, a sliced plan without ownership."""
    rt = nat.get_runtime()
    n_a, n_b = 40, 30

    def create(variant, flags, dtype=nat.SKF_F64, row_begin=0, n_rows=0, part=(0, 2), owned=True):
        rel = dict(row_type=0, col_type=1, flags=flags, known_bound=0 if flags & nat.SKF_REL_ABSENT else 10, row_begin=row_begin,
                   n_rows=n_rows)
        return plan_create_status(rt.lib, [(n_a, 8), (n_b, 6)], [rel], dtype=dtype, variant=variant, part=part,
                                  opt_flags=nat.SKF_OPT_OWNED_ROWS if owned else 0)[0]
    ok, bad = 0, nat.SKF_E_INVALID
    sp0, kn, absent = nat.SKF_REL_SPARSE_CSR, nat.SKF_REL_KNOWN_CSR, nat.SKF_REL_ABSENT
    assert owned_rows('f64', n_a, 0, 2)[:2] == (0, 20) and owned_rows('f64', n_a, 1, 2)[:2] == (20, 20)
    assert owned_rows('bf16', n_a, 1, 2)[:2] == (40, 0)         # (64-aligned chunk: the second rank owns nothing)
    # the owned range, either kind, either rank, either variant that takes the kind
    assert create(nat.SKF_DFMF, sp0, n_rows=20) == ok
    assert create(nat.SKF_DFMF, sp0, row_begin=20, n_rows=20, part=(1, 2)) == ok
    assert create(nat.SKF_DFMC, sp0, n_rows=20) == ok
    assert create(nat.SKF_DFMC, kn, n_rows=20) == ok
    assert create(nat.SKF_DFMC, kn, row_begin=20, n_rows=20, part=(1, 2)) == ok
    assert create(nat.SKF_DFMF, sp0, dtype=nat.SKF_BF16, n_rows=40) == ok              # (n_rows == all rows: rank 0 owns them)
    # a rank without rows: absent
    assert create(nat.SKF_DFMF, sp0 | absent, dtype=nat.SKF_BF16, part=(1, 2)) == ok
    assert create(nat.SKF_DFMC, kn | absent, dtype=nat.SKF_BF16, part=(1, 2)) == ok
    # not the owned range
    assert create(nat.SKF_DFMF, sp0, n_rows=24) == bad
    assert create(nat.SKF_DFMF, sp0, row_begin=4, n_rows=20) == bad
    assert create(nat.SKF_DFMF, sp0, row_begin=20, n_rows=20) == bad                   # (rank 1's rows on rank 0)
    assert create(nat.SKF_DFMF, sp0) == bad                                            # (n_rows = 0: the whole relation)
    assert create(nat.SKF_DFMC, kn, n_rows=24) == bad
    assert create(nat.SKF_DFMC, kn) == bad
    assert create(nat.SKF_DFMF, sp0 | absent) == bad                                   # (absent where rows are owned)
    assert create(nat.SKF_DFMC, kn | absent, part=(1, 2)) == bad
    assert create(nat.SKF_DFMF, sp0, dtype=nat.SKF_BF16, part=(1, 2)) == bad           # (not absent where none is owned)
    assert create(nat.SKF_DFMF, kn, n_rows=20) == bad                                  # (known entries need SKF_DFMC)
    # without ownership: row blocks, slices and part_count > 1 stay refused
    assert create(nat.SKF_DFMF, sp0, n_rows=20, part=(0, 0), owned=False) == bad
    assert create(nat.SKF_DFMF, sp0, n_rows=20, owned=False) == bad
    assert create(nat.SKF_DFMF, sp0, owned=False) == bad
    assert create(nat.SKF_DFMC, kn, n_rows=20, owned=False) == bad
    assert create(nat.SKF_DFMC, kn, owned=False) == bad
    assert create(nat.SKF_DFMF, sp0 | absent, owned=False) == bad


def absent_handover_case():
    """A SKF_REL_ABSENT relation takes no lists: skf_plan_set_known_entries on it is SKF_E_INVALID (bf16, 40 objects, rank 1
    of 2 owns no row)."""
    rt = nat.get_runtime()
    for variant, flag in ((nat.SKF_DFMF, nat.SKF_REL_SPARSE_CSR), (nat.SKF_DFMC, nat.SKF_REL_KNOWN_CSR)):
        tdesc = (nat.TypeDesc * 2)()
        tdesc[0].n_obj, tdesc[0].rank, tdesc[1].n_obj, tdesc[1].rank = 40, 8, 30, 6
        rdesc = (nat.RelationDesc * 1)()
        rdesc[0].row_type, rdesc[0].col_type, rdesc[0].flags = 0, 1, flag | nat.SKF_REL_ABSENT
        opt = nat.Options(nat.SKF_BF16, variant, -1, nat.SKF_ENGINE_MFMA, 1, 2, nat.SKF_OPT_OWNED_ROWS)
        handle = nat._P()
        rt.call('skf_plan_create', 2, tdesc, 1, rdesc, 0, (nat.ThetaDesc * 1)(), C.byref(opt), C.byref(handle))
        try:
            keep = rt.mem.from_host(np.zeros(4, dtype=np.int64))
            with pytest.raises(nat.SkfNativeError) as err:
                rt.call('skf_plan_set_known_entries', handle, 0, keep.ptr, keep.ptr, keep.ptr)
            assert err.value.code == nat.SKF_E_INVALID
        finally:
            rt.lib.skf_plan_destroy(handle)


# ---- 2. the lists a bind builds from a slice ----------------------------------------------------------------------------
def lists_case(dtype, size, parts, unstored, monkeypatch, seed=0, c_a=64, c_b=24, n_a=None):
    """For every rank of `size`: row and column lists of the owned plan == scipy's of csr[begin : begin + count], byte for
    byte, values in the master type, row indices local.  The rows of the LAST rank that owns any hold no entry (a slice with
    nnz = 0), row 7 is full."""
    import scipy.sparse
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    rs = np.random.RandomState(seed)
    n_a, n_b = n_a or N_LISTS['a'], N_LISTS['b']        # (n_a = 120, bf16, 3 ranks: chunks of 64, the third rank owns no row)
    pat = rs.rand(n_a, n_b) < 0.04
    pat[7, :] = True
    pat[:, 5] = False
    pat[7, 5] = True
    owners = [q for q in range(size) if owned_rows(dtype, n_a, q, size)[1] > 0]
    b_e, c_e, _ = owned_rows(dtype, n_a, owners[-1], size)
    if len(owners) > 1:
        pat[b_e:b_e + c_e, :] = False
    # (SKF_BF16 takes known entries as bf16 bits: multiples of 1/8 are exact there; everything else goes up in the master type)
    exact = dtype == 'bf16' and unstored == 'unknown'
    R = np.where(pat, SC.eighths(rs, (n_a, n_b)) + (0.0 if exact else rs.rand(n_a, n_b)), 0.0)
    sp = scipy.sparse.coo_matrix((R[pat], np.nonzero(pat)), shape=R.shape).tocsr()
    sp.sort_indices()
    ke = KnownEntries(sp.indptr, sp.indices, sp.data, sp.shape, unstored=unstored)
    types, n, ranks = ['a', 'b'], {'a': n_a, 'b': n_b}, {'a': c_a, 'b': c_b}
    variant = nat.SKF_DFMF if unstored == 'zero' else nat.SKF_DFMC
    vt = np.float64 if dtype == 'f64' else np.float32
    seen_rows, seen_empty, seen_absent = 0, False, False
    for q in range(size):
        begin, count, _ = owned_rows(dtype, n_a, q, size)
        plan = owned_plan(variant, [('a', 'b', ke, None)], [], types, n, ranks, dtype, None, q, size)
        try:
            if count == 0:
                with pytest.raises(nat.SkfNativeError):         # an absent relation keeps no lists
                    plan.relation_lists(0, False)
                seen_absent = True
                continue
            rp, ri, rv = plan.relation_lists(0, False)
            cp, ci, cv = plan.relation_lists(0, True)
        finally:
            plan.close()
        csr = sp[begin:begin + count]
        csr.sort_indices()
        csc = csr.tocsc()
        csc.sort_indices()
        assert rp.shape == (count + 1,) and cp.shape == (n_b + 1,)
        assert np.array_equal(rp, csr.indptr) and np.array_equal(ri, csr.indices) and np.array_equal(rv, csr.data.astype(vt))
        assert np.array_equal(cp, csc.indptr) and np.array_equal(ci, csc.indices) and np.array_equal(cv, csc.data.astype(vt))
        seen_rows += count
        seen_empty = seen_empty or csr.nnz == 0
    assert seen_rows == n_a and (seen_empty or len(owners) == 1) and seen_absent == (len(owners) < size)


# ---- 3. invalid slices ----------------------------------------------------------------------------------------------------
def invalid_slice_case(which, unstored):
    """Rank 0 of 2 of a graph of 8 x 6 objects owns rows [0, 4): its slice (known_csr_cases.small_lists, already on the
    device: no host check) with an indptr that does not start at 0 (a slice cut out without rebasing), a column out of
    range or descending columns is refused by the validation kernel alone, before anything gathers through it."""
    variant = nat.SKF_DFMF if unstored == 'zero' else nat.SKF_DFMC

    def call(w):
        indptr, idx = KC.small_lists('ok' if w == 'offset' else w)
        if w == 'offset':
            indptr = indptr + 3
        mem = nat.get_runtime().mem
        dev = DeviceKnownEntries(mem.from_host(indptr), mem.from_host(idx), mem.from_host(np.random.RandomState(0).rand(6)), (4, 6),
                                 6, unstored=unstored)
        blk = dict(row_begin=0, n_rows=4, absent=False, masked=False, entries=unstored)
        DevicePlan(['a', 'b'], {'a': 8, 'b': 6}, {'a': 2, 'b': 2}, [('a', 'b', dev, None, blk)], [], variant, part=(0, 2),
                   owned=True).close()
    assert owned_rows('f64', 8, 0, 2)[:2] == (0, 4)
    KC.refused_after_one_launch(call, which)


# ---- whole fits -----------------------------------------------------------------------------------------------------------
def _as_dicts(types, rels, thetas, G0, sparse=(), known=()):
    """(R, M, Theta, G0) dictionaries; `sparse`: relations handed over as stored entries, `known`: as known entries."""
    R, M = {}, {}
    for k, rel in enumerate(rels):
        i, j, data = rel[0], rel[1], rel[2]
        mask = rel[3] if len(rel) > 3 else None
        if k in sparse:
            data, mask = SC.stored_entries(data), None
        elif k in known:
            data, mask = KC.known_entries_of(data, mask), None
        R[i, j], M[i, j] = [data], [mask]
    return R, M, {(t, t): [th] for t, th in thetas}, {(t, t): G0[t] for t in types}


def _final_gather_bytes(dtype, types, n, ranks, size, master):
    """SKF_BF16: the ONE gather of the f32 rows at the end of a call, for the types that travel as bf16 rows."""
    if dtype != 'bf16':
        return 0.0
    return (size - 1) / float(size) * sum(owned_rows(dtype, n[t], 0, size)[2] * size * ranks[t] * 4 for t in types if t not in master)


def _check_exchange(grp, said, iters, final):
    assert len(set(said)) == 1
    assert abs(grp.bytes_sent_per_rank() - iters * said[0] - final) <= 5.0, (grp.bytes_sent_per_rank(), iters * said[0], final)


def _same_on_every_rank(out, types):
    for G, S in out[1:]:
        for t in types:
            np.testing.assert_array_equal(G[t, t], out[0][0][t, t])
        for k in S:
            np.testing.assert_array_equal(S[k][0], out[0][1][k][0])


def dfmf_against_oracle(ranks, size, parts, monkeypatch, iters=4, seed=0):
    """4. f64, DFMF: a-b and b-c CSR-fed (rank 0 of 2 owns rows of 'a' without an entry), a-c dense, a constraint on b."""
    from oracle import dfmf_oracle as orc
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    n = N_FIT
    types, rels, thetas, G0 = SC.fusion_graph(n, ranks, seed, density=(0.05, 0.03), empty_side=True)
    b0, c0, _ = owned_rows('f64', n['a'], 0, size)
    if size == 2:
        assert not rels[0][2][b0:b0 + c0].any()                 # the slice with nnz = 0
    R, _, Theta, G0d = _as_dicts(types, rels, thetas, G0, sparse=(0, 1))
    Rd, _, _, _ = _as_dicts(types, rels, thetas, G0)
    Go, So = orc.dfmf(Rd, Theta, types, ranks, max_iter=iters, G0=G0d)
    sq = []
    out, grp, said = fit_owned('dfmf', R, None, Theta, types, ranks, G0d, iters, size, sqerr=sq)
    what = 'owned CSR-fed f64 DFMF, %d ranks, parts %d vs oracle' % (size, parts)
    for q, (G, S) in enumerate(out):
        for t in types:
            within(relerr(G[t, t], Go[t, t]), 1e-9, '%s: rank %d G_%s' % (what, q, t))
        for (i, j, _) in rels:
            within(relerr(S[i, j][0], So[i, j][0]), 1e-9, '%s: rank %d S_%s%s' % (what, q, i, j))
    _same_on_every_rank(out, types)
    tot = np.sum(np.array(sq), axis=0)
    for k, (i, j, M) in enumerate(rels):
        want = np.sum((M - Go[i, i] @ So[i, j][0] @ Go[j, j].T) ** 2)
        within(abs(tot[k] - want) / want, 1e-8, '%s: summed squared error of relation %d' % (what, k))
    _check_exchange(grp, said, iters, 0.0)


def dfmc_against_oracle(ranks, size, parts, monkeypatch, iters=4):
    """4. f64, DFMC: both masked relations as their known entries, the unmasked b-c relation as its stored entries; the
    comparisons of test_owned_rows_keep_the_lists_of_known_entries."""
    from oracle import dfmf_oracle as orc
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    n = N_FIT
    types, rels, thetas, G0 = K.masked_graph(n, ranks, 0.05, seed=3)
    Rd, Md, Theta, G0d = _as_dicts(types, rels, thetas, G0)
    R, M, _, _ = _as_dicts(types, rels, thetas, G0, sparse=(1,), known=(0, 2))
    Go, So = orc.dfmc(Rd, Md, Theta, types, ranks, max_iter=iters, G0=G0d)
    sq = []
    out, grp, said = fit_owned('dfmc', R, M, Theta, types, ranks, G0d, iters, size, sqerr=sq)
    what = 'owned CSR-fed f64 DFMC, %d ranks, parts %d vs oracle' % (size, parts)
    for q, (G, S) in enumerate(out):
        for t in types:
            within(relerr(G[t, t], Go[t, t]), 1e-9, '%s: rank %d G_%s' % (what, q, t))
        for (i, j, _, _) in rels:
            within(relerr(S[i, j][0], So[i, j][0]), 1e-9, '%s: rank %d S_%s%s' % (what, q, i, j))
    _same_on_every_rank(out, types)
    tot = np.sum(np.array(sq), axis=0)
    eo = orc.relation_errors(Rd, Go, So)
    within(abs(np.sqrt(tot[1]) - eo['b', 'c'][0]) / eo['b', 'c'][0], 1e-8, '%s: error of the unmasked (stored-entry) relation' % what)
    assert np.isfinite(tot).all() and (tot > 0).all()
    _check_exchange(grp, said, iters, 0.0)


def dfmf_csr_against_dense(key, size, parts, monkeypatch, iters=4, seed=0):
    """5. + 6. DFMF, every engine: CSR-fed owned fit against dense-fed owned fit, same graph, world and G0; what the ranks sent."""
    dtype, ranks = RANKS[key]
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    n = N_FIT
    types, rels, thetas, G0 = SC.fusion_graph(n, ranks, seed, density=(0.05, 0.03))
    R, _, Theta, G0d = _as_dicts(types, rels, thetas, G0, sparse=(0, 1))
    Rd, _, _, _ = _as_dicts(types, rels, thetas, G0)
    sq_s, sq_d = [], []
    out_s, grp, said = fit_owned('dfmf', R, None, Theta, types, ranks, G0d, iters, size, dtype=dtype, sqerr=sq_s)
    out_d, _, said_d = fit_owned('dfmf', Rd, None, Theta, types, ranks, G0d, iters, size, dtype=dtype, sqerr=sq_d)
    what = 'owned %s DFMF %s, %d ranks, parts %d: CSR-fed vs dense-fed' % (dtype, key, size, parts)
    _compare(out_s, out_d, sq_s, sq_d, types, rels, sp0_tol(key), what)
    _same_on_every_rank(out_s, types)
    assert said == said_d                               # (the same collectives run: skf_exchange_bytes is unchanged)
    _check_exchange(grp, said, iters, _final_gather_bytes(dtype, types, n, ranks, size, master=('b',)))    # ('b': the constraint)


def dfmc_csr_against_dense(key, size, parts, monkeypatch, iters=4):
    """5. + 6. DFMC, every engine: the masked relations as known entries against the same relations as dense + mask, whose
    owned plans keep the lists of the mask (SKF_DFMC_SPARSE=1): the same lists, hence also bit for bit."""
    dtype, ranks = RANKS[key]
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    monkeypatch.setenv('SKF_DFMC_SPARSE', '1')
    n = N_FIT
    types, rels, thetas, G0 = K.masked_graph(n, ranks, 0.05, seed=3)
    if dtype == 'bf16':                                 # (both hand-overs then hold the same bf16 values)
        rels = [(i, j, nat.from_bf16_bits(nat.to_bf16_bits(R)).astype(np.float64), M) for i, j, R, M in rels]
    Rd, Md, Theta, G0d = _as_dicts(types, rels, thetas, G0)
    R, M, _, _ = _as_dicts(types, rels, thetas, G0, known=(0, 2))
    sq_s, sq_d = [], []
    out_s, grp, said = fit_owned('dfmc', R, M, Theta, types, ranks, G0d, iters, size, dtype=dtype, sqerr=sq_s)
    out_d, _, said_d = fit_owned('dfmc', Rd, Md, Theta, types, ranks, G0d, iters, size, dtype=dtype, sqerr=sq_d)
    what = 'owned %s DFMC %s, %d ranks, parts %d: CSR-fed vs mask-fed lists' % (dtype, key, size, parts)
    _compare(out_s, out_d, sq_s, sq_d, types, rels, TOL_KNOWN[dtype], what)
    for (Gs, Ss), (Gd, Sd) in zip(out_s, out_d):
        for t in types:
            assert np.array_equal(Gs[t, t], Gd[t, t]), '%s: G_%s differs' % (what, t)
        for k in Ss:
            assert np.array_equal(Ss[k][0], Sd[k][0]), '%s: S_%s differs' % (what, k)
    assert np.array_equal(np.array(sq_s), np.array(sq_d))
    _same_on_every_rank(out_s, types)
    assert said == said_d
    _check_exchange(grp, said, iters, _final_gather_bytes(dtype, types, n, ranks, size, master=('a', 'b', 'c')))


def _compare(out_s, out_d, sq_s, sq_d, types, rels, tol, what):
    for q, ((Gs, Ss), (Gd, Sd)) in enumerate(zip(out_s, out_d)):
        for t in types:
            assert np.isfinite(Gs[t, t]).all()
            within(relerr(Gs[t, t], Gd[t, t]), tol[0], '%s, rank %d G_%s' % (what, q, t))
        for rel in rels:
            i, j = rel[0], rel[1]
            within(relerr(Ss[i, j][0], Sd[i, j][0]), tol[1], '%s, rank %d S_%s%s' % (what, q, i, j))
    Es, Ed = np.sum(np.array(sq_s), axis=0), np.sum(np.array(sq_d), axis=0)
    assert np.isfinite(Es).all() and (Ed > 0).all()
    within(np.max(np.abs(Es - Ed) / Ed), tol[2], '%s, summed squared errors' % what)


# ---- 7. never expanded ---------------------------------------------------------------------------------------------------
def never_expanded_plans(monkeypatch, iterate=True):
    """20 000 x 16 000, ~64 000 entries, ranks 128 / 64, f32, 2 ranks through owned_plan: toarray() / mask() raise, and a
    rank's workspace stays below a quarter of the dense f32 relation (a condition: lists, factors and the partial Q of this
    graph are tens of MB against 1.28 GB)."""
    n_r, n_c, per_row = 20000, 16000, 4
    rs = np.random.RandomState(0)
    step = n_c // per_row
    cols = rs.randint(0, step, (n_r, per_row), dtype=np.int32) + (np.arange(per_row, dtype=np.int32) * step)[None, :]
    keep = rs.rand(n_r, per_row) < 0.73                 # strictly ascending columns in every row, 1 to 4 of them
    keep[:, 0] = True
    counts = keep.sum(axis=1)
    indptr = np.zeros(n_r + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    vals = rs.randint(1, 64, int(indptr[-1])) / 8.0
    ke = KnownEntries(indptr, cols[keep], vals, (n_r, n_c), unstored='zero')
    assert 60000 <= ke.known <= 68000

    def refuse(*a, **k):
        raise AssertionError('a relation given as its entries was expanded')
    monkeypatch.setattr(KnownEntries, 'toarray', refuse)
    monkeypatch.setattr(KnownEntries, 'mask', refuse)
    types, n, ranks = ['row', 'col'], {'row': n_r, 'col': n_c}, {'row': 128, 'col': 64}
    size = 2
    rt = nat.get_runtime()
    plans = [owned_plan(nat.SKF_DFMF, [('row', 'col', ke, None)], [], types, n, ranks, 'f32', None, q, size) for q in range(size)]
    try:
        for p in plans:
            assert p.workspace_bytes < n_r * n_c * 4 // 4, p.workspace_bytes
        if not iterate:
            return
        grp = ThreadGroup(size, sync=rt.mem.synchronize, serial=True)
        G0 = {t: (rs.rand(n[t], ranks[t]) * 0.1 + 0.01) for t in types}
        for q, p in enumerate(plans):
            p.attach_callback_comm(q, size, grp.collective)
            for t in types:
                p.set_factor(t, G0[t])
        grp.run(plans, lambda p: p.iterate_dist(2))
        errs = [sum(p.relation_sqerr(0) for p in plans)]
        grp.run(plans, lambda p: p.iterate_dist(1))
        errs.append(sum(p.relation_sqerr(0) for p in plans))
        for t in types:
            G = [p.get_factor(t) for p in plans]
            assert np.isfinite(G[0]).all() and np.array_equal(G[0], G[1])
        assert np.isfinite(errs).all() and errs[1] < errs[0], errs
    finally:
        for p in plans:
            p.close()


# Dfmc, ratings graph 300 x 250 at 5 % known, ranks 70 / 12 / 4, 4 iterations: shard='owned' against shard='runs' of the MASK
# form of the same data with SKF_DFMC_SPARSE=1 (lists on both sides) on the commit before this hand-over existed -- the two
# schedules differ by f64 rounding times the conditioning of the Gram matrices, whatever the form.  Factors of users / movies
# / genres, backbones of ratings / genres; worst of the host emulator and the MI355X.  The wide case is held to 10 x these.
WIDE_MASK_FORM = {'factors': (3.73e-10, 1.13e-9, 7.75e-12), 'backbones': (1.38e-7, 4.39e-10)}


def never_expanded_api(cls, monkeypatch, n=(300, 250), wide=False):
    """Dfmf(shard='owned', sparse_relations=True) / Dfmc(shard='owned') on a relation given with unstored='unknown', one
    process: toarray / todense / dense_data of the relation raise, and the fit is the shard='runs' fit of the same graph to
    1e-11 (f64: the bound sharded_fits_of_a_single_process_are_the_plain_fit uses).  The two fits run different schedules
    (the owned one and the single-device one), so they differ by f64 rounding times the conditioning of the Gram matrices: the
    ratings graph at 5 % known is held to 1e-11 at ranks 8 / 6 / 4, where the mask form of the same data -- lists on both
    sides, code from before this hand-over -- differs by 5e-13 between the two shards.  `wide` (Dfmc): ranks 70 / 12 / 4,
    the wide list kernels, where that mask form itself differs by up to 1.1e-9 (factors) and 1.4e-7 (backbones): every
    factor and backbone is held to 10 x its own figure of WIDE_MASK_FORM."""
    import sparse_dfmf_api_cases as AC
    import known_csr_api_cases as KA
    from skfusion_amd.fusion import Dfmf

    def refuse(*a, **k):
        raise AssertionError('an eligible sparse relation was expanded')
    kw = dict(max_iter=4, init_type='random_vcol', random_state=0, dtype='f64')
    ranks = (70, 12, 4) if cls is Dfmf or wide else (8, 6, 4)
    if cls is Dfmf:
        sp = AC.counts(n[0], n[1], 0.02, 3)
        kw['sparse_relations'] = True
        g_own = AC.graph(AC.forbid_toarray(monkeypatch, sp.copy()), ranks=ranks)
        g_run = AC.graph(sp, ranks=ranks)
    else:
        sp, _ = KA.ratings(n[0], n[1], 0.05, 7)
        g_own = KA.graph(AC.forbid_toarray(monkeypatch, sp.copy()), ranks=ranks, unstored='unknown')[0]
        g_run = KA.graph(sp, ranks=ranks, unstored='unknown')[0]
    for rel in g_own.relations:
        if rel.row_type != rel.col_type and not isinstance(rel.data, np.ndarray):
            monkeypatch.setattr(rel, 'dense_data', refuse)
    own = cls(shard='owned', **kw).fuse(g_own)
    run = cls(shard='runs', **kw).fuse(g_run)
    what = "%s shard='owned' vs 'runs' through the API%s" % (cls.__name__, ', ranks 70 / 12 / 4' if wide else '')
    for k, (ta, tb) in enumerate(zip(g_own.object_types, g_run.object_types)):
        bound = 10.0 * WIDE_MASK_FORM['factors'][k] if wide else 1e-11
        within(relerr(own.factor(ta), run.factor(tb)), bound, '%s, factor of %s' % (what, ta.name))
    for k, (ra, rb) in enumerate(zip(g_own.relations, g_run.relations)):
        bound = 10.0 * WIDE_MASK_FORM['backbones'][k] if wide else 1e-11
        within(relerr(own.backbone(ra), run.backbone(rb)), bound, '%s, backbone of %s' % (what, ra.name))


# ---- 9. stopping ----------------------------------------------------------------------------------------------------------
def stopping_case(size=2, seed=0):
    """`stopping_system` on a CSR-fed owned fit: the existing host loop (_dfmf._host_loop, what run_fit_owned drives), one
    iteration of the thread ranks per step and the ranks' squared errors summed, stops at the iteration at which the oracle
    stops.  The threshold sits half-way between two consecutive decrements of the oracle's own system error."""
    from oracle import dfmf_oracle as orc
    n, ranks = N_FIT, {'a': 16, 'b': 12, 'c': 8}
    types, rels, thetas, G0 = SC.fusion_graph(n, ranks, seed, density=(0.05, 0.03))
    R, _, Theta, G0d = _as_dicts(types, rels, thetas, G0, sparse=(0, 1))
    Rd, _, _, _ = _as_dicts(types, rels, thetas, G0)
    trace = []
    orc.dfmf(Rd, Theta, types, ranks, max_iter=12, G0=G0d,
             callback=lambda G, S, it: trace.append(sum(sum(v) for v in orc.relation_errors(Rd, G, S).values())))
    ds = -np.diff(trace)
    eps = 0.5 * (ds[5] + ds[6])
    assert ds[5] > eps * 1.005 and ds[6] < eps * 0.995
    want = []
    Go, So = orc.dfmf(Rd, Theta, types, ranks, max_iter=30, G0=G0d, stopping_system=eps, callback=lambda G, S, it: want.append(it))
    assert 2 < len(want) < 30
    rel_list, th = flatten_relations(R, None), flatten_thetas(Theta)
    nn = count_objects(types, R)
    rt = nat.get_runtime()
    grp = ThreadGroup(size, sync=rt.mem.synchronize, serial=True)
    plans = [owned_plan(nat.SKF_DFMF, rel_list, th, types, nn, ranks, 'f64', None, q, size) for q in range(size)]
    try:
        for q, p in enumerate(plans):
            p.attach_callback_comm(q, size, grp.collective)
            for t in types:
                p.set_factor(t, G0d[t, t])
        seen = []
        _host_loop(lambda: grp.run(plans, lambda p: p.iterate_dist(1)),
                   lambda idx: [sum(p.relation_sqerr(k) for p in plans) for k in idx],
                   rel_list, 30, None, eps, False, seen.append)
        assert seen == want, (seen, want)
        for p in plans:
            for t in types:
                within(relerr(p.get_factor(t), Go[t, t]), 1e-9, 'owned CSR-fed fit stopped by stopping_system vs oracle, G_%s' % t)
    finally:
        for p in plans:
            p.close()
