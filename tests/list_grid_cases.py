"""Every entry-list form of the engine at outer sizes that are no multiple of the 4 objects of a workgroup, fewer than one
workgroup's and fewer than one group of 8 workgroups' (srp_grid / srp_segment in csrc/skf_known.h, srp_pass in
csrc/skf_stages.inc): the grid, the part a workgroup takes and the number of error partials the plan reserved room for
are decided in one place, and these are the shapes at which that decision could go wrong -- the SAME cases on the host
emulator and on the GPU.

Nothing here has a model or a bound of its own: every case is a call of the case function of the form's own module, at its
own tolerances, with the shapes below.  One iteration runs, the contractions (the fold-in: the target's factor) and
relation_sqerr are held to the host.  A capacity check that refused the error pass (SKF_E_STATE: the layout reserved fewer
partial slots than the launch writes) fails the case by name."""
import numpy as np

import skfusion_amd._native as nat
from helpers import relerr, within

import known_cases as K
import sparse_dfmf_cases as SD
import filled_entries_cases as FE
import sparse_foldin_cases as SF

# (n_i, n_j): 5 rows are two workgroups of which the second holds one object, 33 columns 9 workgroups (one group of 8 and a
# ninth); 1 x 9: a single object, 3 workgroups.  With 8 parts every workgroup of a group is a part of the same 4 objects.
SHAPES = [(5, 33), (1, 9)]
PARTS = [1, 8]
N_ONES = (69, 333)          # 0/1 relation: 18 workgroups of rows (two groups of 8 and a quarter), 84 of columns


def ranks_of(rank):
    """(c_a, c_b) of the two-type cases: `rank` is the row type's (the width of the known-entry passes and of Q), the column
    type's stays at 3, well below n_j of both shapes.  With c_a >= n_i AND c_b >= n_j the first backbone reproduces the
    relation exactly (one short of n_j: nearly), the residuals the known-entry passes multiply are zero and the squared
    error vanishes -- nothing would be left to compare."""
    return rank, min(rank, 3)


def scratch_sufficed(case, *args, **kw):
    """Run `case`; an SKF_E_STATE out of the library (the error partials outgrew the slots the layout reserved) is named."""
    try:
        return case(*args, **kw)
    except nat.SkfNativeError as exc:
        assert exc.code != nat.SKF_E_STATE, 'the plan\'s scratch did not hold the pass: %s' % exc
        raise


def known_case(shape, rank, dtype, parts, what, monkeypatch):
    """Known entries of a masked relation (DFMC): A = P S^T, Q and the squared error, known_cases.list_case."""
    return scratch_sufficed(K.list_case, shape[0], shape[1], *ranks_of(rank), dtype, parts, 'heavy', what, monkeypatch, seed=parts)


def stored_case(shape, rank, dtype, parts, what, monkeypatch):
    """Stored entries, zero elsewhere (DFMF): P, Q and the squared error, sparse_dfmf_cases.pass_case; a fully stored row
    and column, so that every part of every list holds entries."""
    return scratch_sufficed(SD.pass_case, shape[0], shape[1], *ranks_of(rank), dtype, parts, 'full', what, monkeypatch, seed=parts)


def filled_case(shape, rank, dtype, parts, what, monkeypatch):
    """Stored entries with a rank-one fill: the same through filled_entries_cases.pass_case."""
    return scratch_sufficed(FE.pass_case, shape[0], shape[1], *ranks_of(rank), dtype, parts, 'full', what, monkeypatch, seed=parts)


def ones_case(ranks, parts, pattern, what, monkeypatch):
    """A sparse 0/1 relation as lists over bf16 rows: P and Q, known_cases.ones_case."""
    return scratch_sufficed(K.ones_case, N_ONES[0], N_ONES[1], ranks[0], ranks[1], parts, pattern, what, monkeypatch, seed=parts,
                            lengths=(1, 4, 5, 16, 17))


def fold_case(shape, rank, dtype, what, seed=0):
    """Fold-in lists (no parts): shape[0] new objects through a target x partner and a partner x target relation of
    shape[1] partners each.  One iteration against the f64 host (f64: the 1e-9 of sparse_foldin_cases.whole_case; the other
    engines: finite -- their bound there is a dense-fed plan's own deviation, which says nothing about lists) and
    relation_sqerr of both relations against sparse_foldin_cases.sqerr_ratio."""
    n_t, n_p = shape
    n = {'t': n_t, 'a': n_p, 'b': n_p}
    ranks = {'t': rank, 'a': rank, 'b': rank}
    rs = np.random.RandomState(seed)
    pats = [K.edge_mask(n_t, n_p, 'full', seed, bg=0.2), K.edge_mask(n_p, n_t, 'heavy', seed + 1)]
    rels = [('t', 'a', np.where(pats[0], SF.signed_eighths(rs, (n_t, n_p)), 0.0), pats[0]),
            ('b', 't', np.where(pats[1], SF.signed_eighths(rs, (n_p, n_t)), 0.0), pats[1])]
    f32 = (lambda a: K.store_round(a, 'f32')) if dtype != 'f64' else (lambda a: a)
    Gp = {o: f32(rs.rand(n[o], ranks[o]) + 0.1) for o in ('a', 'b')}
    S = [f32(rs.rand(ranks[i], ranks[j]) * 2.0 - 0.6) for i, j, _, _ in rels]
    G0 = f32(rs.rand(n_t, rank) + 0.1)

    def run():
        plan = SF.make_plan(dtype, n, ranks, rels, None, Gp, S, G0, True)
        try:
            plan.iterate(1)
            return plan.get_factor('t'), [plan.relation_sqerr(k) for k in range(len(rels))]
        finally:
            plan.close()

    Gt, sq = scratch_sufficed(run)
    assert np.isfinite(Gt).all(), what
    out = {}
    if dtype == 'f64':
        want = SF.oracle_fold(rels, None, ranks, Gp, S, G0, 1)
        out['factor'] = within(relerr(Gt, want), 1e-9, '%s: list-fed f64 fold-in vs oracle, one iteration' % what)
    for k, (i, j, R, pat) in enumerate(rels):
        Sk = np.asarray(S[k], dtype=np.float64)
        if i == 't':
            r = SF.sqerr_ratio(dtype, R, pat, Gt, Sk, Gp[j], sq[k], n_t, n[j], rank, rank)
        else:
            r = SF.sqerr_ratio(dtype, R.T, pat.T, Gt, Sk.T, Gp[i], sq[k], n_t, n[i], rank, rank)
        out['sqerr %d' % k] = within(r, 1.0, '%s: relation_sqerr of relation %d (%s x %s), |delta| / model bound' % (what, k, i, j))
    return out
