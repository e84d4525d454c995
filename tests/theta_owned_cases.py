"""Sparse constraints of ownership-sharded fits (SKF_OPT_OWNED_ROWS | SKF_OPT_THETA_OWNED_ROWS, `shard='owned'`): every rank
hands its plan the CSR of the OWNED rows of the constrained type over all columns, never the whole constraint and never a
dense form -- the SAME cases on the host emulator and on the GPU.  Ranks are threads of this process on one device
(helpers.fit_owned / helpers.ThreadGroup).

Bounds.  The anchor is bit identity (np.array_equal) with the DENSE-fed owned fit, code from before this hand-over existed:
that plan compacts the ndarray to the lists of the whole matrix and launches the constraint kernels on the owned sub-range;
the slice holds the same rows, cut at the same places.  f64 against the oracle: 1e-9 on G and S, what
test_owned_sharding.py holds owned fits to.  No other numeric bound appears here."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, DeviceKnownEntries, KnownEntries, owned_rows, launch_count
from skfusion_amd.fusion.decomposition._dfmf import owned_plan
from helpers import relerr, within, fit_owned, ThreadGroup

import known_cases as K
import known_csr_cases as KC
import theta_csr_cases as TC

N_HUB = 300
# HUB_LENGTHS in another order: the rows LONGER than 64 entries (the ones the hub kernels take at SKF_THETA_HUB_ROW=64) are
# rows 18, 93, 168 and 281 of 300 -- on both sides of every boundary of 2 and 3 owners in every engine
SPREAD_LENGTHS = (299, 0, 65, 1, 128, 63, 64, 129)
assert sorted(SPREAD_LENGTHS) == sorted(TC.HUB_LENGTHS)


def boundaries(dtype, n, size):
    """First rows of the owners 1 .. size - 1 that own any row."""
    return [b for b, cnt, _ in (owned_rows(dtype, n, q, size) for q in range(1, size)) if cnt > 0]


def csr_of(theta):
    sp = scipy.sparse.csr_matrix(np.asarray(theta, dtype=np.float64))
    sp.sort_indices()
    return sp


# ---- 1. creation: the status of skf_plan_create alone ------------------------------------------------------------------
def create_status(lib, nnz, keep, variant=nat.SKF_DFMF, dtype=nat.SKF_F64, part=(0, 2), flags=None, theta_type=0, n_a=40):
    """Status of skf_plan_create for n_a x 30 objects, the dense row block of the owned range of type 0 (or an absent one)
    and one constraint given as its entries.  No HIP call is made before the validation answers."""
    flags = (nat.SKF_OPT_OWNED_ROWS | nat.SKF_OPT_THETA_OWNED_ROWS) if flags is None else flags
    tdesc = (nat.TypeDesc * 2)()
    tdesc[0].n_obj, tdesc[0].rank, tdesc[1].n_obj, tdesc[1].rank = n_a, 8, 30, 6
    rdesc = (nat.RelationDesc * 1)()
    rdesc[0].row_type, rdesc[0].col_type, rdesc[0].data, rdesc[0].ld = 0, 1, keep, 30
    if flags & nat.SKF_OPT_OWNED_ROWS:
        begin, count, _ = owned_rows(dtype, n_a, part[0], part[1])
        if count:
            rdesc[0].row_begin, rdesc[0].n_rows = begin, count
        else:
            rdesc[0].data, rdesc[0].flags = None, nat.SKF_REL_ABSENT
    hdesc = (nat.ThetaDesc * 1)()
    hdesc[0].type, hdesc[0].data, hdesc[0].ld, hdesc[0].nnz = theta_type, None, 0, nnz
    opt = nat.Options(dtype, variant, 0 if variant == nat.SKF_TRANSFORM else -1, nat.SKF_ENGINE_MFMA, part[0], part[1], flags)
    handle = nat._P()
    try:
        return lib.skf_plan_create(2, tdesc, 1, rdesc, 1, hdesc, C.byref(opt), C.byref(handle))
    finally:
        if handle.value:
            lib.skf_plan_destroy(handle)


def creation_cases(lib, keep):
    """With the flag: the owned slice is accepted -- either rank, a rank owning no row (nnz = 0), DFMF and DFMC, f64 and
    bf16 --; refused: the flag without SKF_OPT_OWNED_ROWS, nnz < 0, more than 2e9 entries, a type out of range,
    SKF_TRANSFORM.  Without the flag: theta_csr_cases.creation_cases, unchanged."""
    ok, bad = 0, nat.SKF_E_INVALID
    assert nat.SKF_OPT_THETA_OWNED_ROWS == 2
    assert create_status(lib, 10, keep) == ok
    assert create_status(lib, 10, keep, part=(1, 2)) == ok
    assert create_status(lib, 0, keep) == ok                                            # a slice without entries
    assert create_status(lib, 10, keep, variant=nat.SKF_DFMC) == ok
    assert create_status(lib, 10, keep, dtype=nat.SKF_BF16) == ok
    assert create_status(lib, 10, keep, variant=nat.SKF_DFMC, dtype=nat.SKF_BF16) == ok
    assert owned_rows('bf16', 40, 1, 2)[:2] == (40, 0)
    assert create_status(lib, 0, keep, dtype=nat.SKF_BF16, part=(1, 2)) == ok          # this rank owns no row of the type
    assert create_status(lib, 800, keep) == ok                                          # a full slice: lists whatever the density
    assert create_status(lib, 10, keep, flags=nat.SKF_OPT_THETA_OWNED_ROWS, part=(0, 0)) == bad
    assert b'SKF_OPT_OWNED_ROWS' in lib.skf_last_error()
    assert create_status(lib, 10, keep, flags=nat.SKF_OPT_THETA_OWNED_ROWS) == bad      # (a sliced plan without ownership)
    assert create_status(lib, -1, keep) == bad
    assert create_status(lib, 2000000001, keep) == bad
    assert b'2e9' in lib.skf_last_error()
    assert create_status(lib, 10, keep, theta_type=2) == bad
    assert create_status(lib, 10, keep, variant=nat.SKF_TRANSFORM) == bad
    # without the flag an owned plan refuses, with the message it always gave
    assert create_status(lib, 10, keep, flags=nat.SKF_OPT_OWNED_ROWS) == bad
    assert b'constraint 0' in lib.skf_last_error()
    TC.creation_cases(lib, keep)


# ---- 2. the lists a bind keeps --------------------------------------------------------------------------------------------
def lists_case(dtype, size, monkeypatch, n=N_HUB, c=5):
    """constraint_lists(0) of every rank == scipy's csr[begin : begin + count], byte for byte, values in the master type."""
    monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    monkeypatch.setenv('SKF_THETA_HUB_ROW', '64')
    types, nn, ranks, rels, th, _ = TC.hub_graph(n, c, TC.HUB_LENGTHS)
    sp = csr_of(th)
    ke = KnownEntries(sp.indptr, sp.indices, sp.data, sp.shape, unstored='zero')
    vt = np.float64 if dtype == 'f64' else np.float32
    seen, empty_rank = 0, False
    for q in range(size):
        begin, count, _ = owned_rows(dtype, n, q, size)
        plan = owned_plan(nat.SKF_DFMF, rels, [('b', ke)], types, nn, ranks, dtype, None, q, size)
        try:
            rp, ci, vv = plan.constraint_lists(0)
        finally:
            plan.close()
        want = sp[begin:begin + count]
        want.sort_indices()
        assert rp.shape == (count + 1,) and rp.dtype == np.int64 and ci.dtype == np.int32 and vv.dtype == vt
        assert rp.tobytes() == want.indptr.astype(np.int64).tobytes(), 'rank %d of %d: indptr' % (q, size)
        assert ci.tobytes() == want.indices.astype(np.int32).tobytes(), 'rank %d of %d: indices' % (q, size)
        assert vv.tobytes() == want.data.astype(vt).tobytes(), 'rank %d of %d: values' % (q, size)
        seen += count
        empty_rank = empty_rank or count == 0
        if count == 0:
            assert rp.tolist() == [0] and ci.size == 0 and vv.size == 0
    assert seen == n
    return empty_rank


def dense_fed_lists_case(dtype, monkeypatch):
    """The accessor on the path from before it existed: a dense-fed, compacted constraint keeps scipy's CSR of the dense
    matrix (whole matrix, one device); a constraint kept dense has no lists."""
    monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    types, nn, ranks, rels, th, _ = TC.hub_graph(N_HUB, 5, TC.HUB_LENGTHS)
    vt = np.float64 if dtype == 'f64' else np.float32
    sp = csr_of(th)
    plan = DevicePlan(types, nn, ranks, rels, [('b', th)], nat.SKF_DFMF, dtype=dtype)
    try:
        rp, ci, vv = plan.constraint_lists(0)
    finally:
        plan.close()
    assert rp.tobytes() == sp.indptr.astype(np.int64).tobytes() and ci.tobytes() == sp.indices.astype(np.int32).tobytes()
    assert vv.tobytes() == sp.data.astype(vt).tobytes()
    full = np.where(np.random.RandomState(0).rand(N_HUB, N_HUB) < 0.5, 0.25, 0.0)
    plan = DevicePlan(types, nn, ranks, rels, [('b', full)], nat.SKF_DFMF, dtype=dtype)
    try:
        with pytest.raises(nat.SkfNativeError) as err:
            plan.constraint_lists(0)
        assert err.value.code == nat.SKF_E_INVALID
        with pytest.raises(nat.SkfNativeError):
            plan.constraint_lists(1)
    finally:
        plan.close()


# ---- 3. invalid slices ----------------------------------------------------------------------------------------------------
def small_slice(which):
    """Six entries of the rows [0, 4) of a constraint on 8 objects: canonical ('ok'), or cut out without rebasing the
    indptr, with a column out of range, with a descending pair."""
    indptr = np.array([0, 2, 4, 4, 6], dtype=np.int64)
    idx = np.array([1, 3, 0, 2, 4, 7], dtype=np.int32)
    if which == 'offset':
        indptr = indptr + 3
    elif which == 'range':
        idx[3] = 8                                      # column 8 of 8
    elif which == 'descending':
        idx[2], idx[3] = 2, 0
    else:
        assert which == 'ok'
    return indptr, idx


def invalid_slice_case(which):
    """Rank 0 of 2 owns rows [0, 4) of 8 objects; its slice is already on the device (no host check): the validation kernel
    alone refuses it at bind -- one launch, SKF_E_INVALID, the message names the constraint --, before anything gathers
    through it or iterates."""
    said = []

    def call(w):
        indptr, idx = small_slice(w)
        mem = nat.get_runtime().mem
        dev = DeviceKnownEntries(mem.from_host(indptr), mem.from_host(idx), mem.from_host(np.full(6, 0.25)), (4, 8), 6,
                                 unstored='zero')
        blk = dict(row_begin=0, n_rows=4, absent=False, masked=False)
        try:
            DevicePlan(['a', 'b'], {'a': 8, 'b': 6}, {'a': 2, 'b': 2}, [('a', 'b', np.ones((4, 6)), None, blk)], [('a', dev)],
                       nat.SKF_DFMF, part=(0, 2), owned=True).close()
        except nat.SkfNativeError as exc:
            said.append(str(exc))
            raise
    assert owned_rows('f64', 8, 0, 2)[:2] == (0, 4)
    KC.refused_after_one_launch(call, which)
    assert len(said) == 1 and 'constraint 0' in said[0]


# ---- 4. the anchor: the bits of the dense-fed owned fit -------------------------------------------------------------------
def _same_on_every_rank(out, types):
    for G, S in out[1:]:
        for t in types:
            np.testing.assert_array_equal(G[t, t], out[0][0][t, t])
        for k in S:
            np.testing.assert_array_equal(S[k][0], out[0][1][k][0])


def _same_bits(out_e, out_d, what):
    assert len(out_e) == len(out_d)
    for q, ((Ge, Se), (Gd, Sd)) in enumerate(zip(out_e, out_d)):
        for k in Ge:
            assert np.isfinite(Ge[k]).all(), '%s: rank %d G_%s not finite' % (what, q, k[0])
            assert np.array_equal(Ge[k], Gd[k]), '%s: rank %d G_%s differs' % (what, q, k[0])
        for k in Se:
            assert np.array_equal(Se[k][0], Sd[k][0]), '%s: rank %d S_%s%s differs' % (what, q, k[0], k[1])


def hub_rows_straddle(dtype, size, lengths, hub_row=64):
    """The rows of hub_graph with their own lengths lie on both sides of every ownership boundary of this world; with
    SPREAD_LENGTHS so do the rows the hub kernels take (longer than `hub_row` entries)."""
    rows = TC.hub_rows(N_HUB, len(lengths))
    cuts = boundaries(dtype, N_HUB, size)
    assert cuts, 'a world of %d owners has no boundary inside %d rows' % (size, N_HUB)
    for b in cuts:
        assert min(rows) < b <= max(rows), (dtype, size, b, rows)
    if lengths == SPREAD_LENGTHS:
        long_rows = [r for r, L in zip(rows, lengths) if L > hub_row]
        for b in cuts:
            assert min(long_rows) < b <= max(long_rows), (dtype, size, b, long_rows)


def hub_bits_case(dtype, c, size, hub, monkeypatch, lengths=TC.HUB_LENGTHS, iters=3):
    """DFMF, 3 iterations: entries-fed (every rank its slice) against dense-fed (every rank the ndarray), same world, G0."""
    monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    monkeypatch.setenv('SKF_THETA_HUB_ROW', str(hub))
    hub_rows_straddle(dtype, size, lengths)
    types, nn, ranks, rels, th, G0 = TC.hub_graph(N_HUB, c, lengths)
    R = {('b', 'p'): [rels[0][2]]}
    G0d = {(t, t): G0[t] for t in types}
    out_d, _, said_d = fit_owned('dfmf', R, None, {('b', 'b'): [th]}, types, ranks, G0d, iters, size, dtype=dtype)
    out_e, _, said_e = fit_owned('dfmf', R, None, {('b', 'b'): [TC.entries_of(th)]}, types, ranks, G0d, iters, size, dtype=dtype)
    what = 'owned %s DFMF c %d, %d ranks, hub %d: constraint as entries vs ndarray' % (dtype, c, size, hub)
    _same_bits(out_e, out_d, what)
    _same_on_every_rank(out_e, ['b', 'p'])
    assert said_e == said_d and len(set(said_e)) == 1           # skf_exchange_bytes is unchanged
    return out_e


def dfmc_bits_case(size, monkeypatch, iters=3):
    """DFMC on known_cases.masked_graph, its constraint on b as entries against the same constraint as ndarray."""
    n, ranks = {'a': 200, 'b': 140, 'c': 130}, {'a': 8, 'b': 12, 'c': 6}
    types, rels, thetas, G0 = K.masked_graph(n, ranks, 0.05, seed=3)
    R = {(i, j): [d] for i, j, d, _ in rels}
    M = {(i, j): [m] for i, j, _, m in rels}
    G0d = {(t, t): G0[t] for t in types}
    th = thetas[0][1]
    assert 0 < np.count_nonzero(th) <= n['b'] * n['b'] // 16                # (the dense-fed plan compacts it)
    out_d, _, said_d = fit_owned('dfmc', R, M, {('b', 'b'): [th]}, types, ranks, G0d, iters, size)
    out_e, _, said_e = fit_owned('dfmc', R, M, {('b', 'b'): [TC.entries_of(th)]}, types, ranks, G0d, iters, size)
    _same_bits(out_e, out_d, 'owned f64 DFMC, %d ranks: constraint as entries vs ndarray' % size)
    _same_on_every_rank(out_e, types)
    assert said_e == said_d


def launch_counts_case(dtype, size, monkeypatch, c=65, iters=1):
    """Launches of one iteration per rank, split (SKF_THETA_HUB_ROW=64) and unsplit (0), entries-fed and dense-fed: the two
    forms launch the same kernels on every rank, and splitting adds the two hub kernels exactly where the rank owns a row
    longer than 64 entries.  Returns {(hub, form): [launches of every rank]}."""
    monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    types, nn, ranks, rels, th, G0 = TC.hub_graph(N_HUB, c, SPREAD_LENGTHS)
    rt = nat.get_runtime()
    out = {}
    for hub in (64, 0):
        monkeypatch.setenv('SKF_THETA_HUB_ROW', str(hub))
        for form, theta in (('entries', TC.entries_of(th)), ('dense', th)):
            grp = ThreadGroup(size, sync=rt.mem.synchronize, serial=True)
            plans = [owned_plan(nat.SKF_DFMF, rels, [('b', theta)], types, nn, ranks, dtype, None, q, size) for q in range(size)]
            counts = {}
            try:
                for q, p in enumerate(plans):
                    p.attach_callback_comm(q, size, grp.collective)
                    for t in types:
                        p.set_factor(t, G0[t])

                def drive(p):
                    before = launch_count()
                    p.iterate_dist(iters)
                    counts[plans.index(p)] = launch_count() - before
                grp.run(plans, drive)
            finally:
                for p in plans:
                    p.close()
            out[hub, form] = [counts[q] for q in range(size)]
    rows = TC.hub_rows(N_HUB, len(SPREAD_LENGTHS))
    for q in range(size):
        begin, count, _ = owned_rows(dtype, N_HUB, q, size)
        owns_long = any(begin <= r < begin + count and L > 64 for r, L in zip(rows, SPREAD_LENGTHS))
        for hub in (64, 0):
            assert out[hub, 'entries'][q] == out[hub, 'dense'][q], (dtype, size, hub, q, out)
        assert out[64, 'entries'][q] - out[0, 'entries'][q] == (2 * iters if owns_long else 0), (dtype, size, q, out)
    print('launches per rank, %s, %d ranks, %d iteration(s): split %r, unsplit %r' % (dtype, size, iters, out[64, 'entries'],
                                                                                   out[0, 'entries']))
    return out


# ---- 5. f64 against the oracle ----------------------------------------------------------------------------------------------
DENSE_LENGTHS = tuple(130 + k for k in range(40))       # 40 rows of about 150 entries: more than n^2 / 16 entries in all


def oracle_case(size, monkeypatch, lengths=TC.HUB_LENGTHS, iters=3, c=65):
    from oracle import dfmf_oracle as orc
    monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    monkeypatch.setenv('SKF_THETA_HUB_ROW', '64')
    types, nn, ranks, rels, th, G0 = TC.hub_graph(N_HUB, c, lengths)
    if lengths == DENSE_LENGTHS:                        # no dense-fed plan would keep this one as lists
        assert np.count_nonzero(th) > N_HUB * N_HUB // 16
    R = {('b', 'p'): [rels[0][2]]}
    G0d = {(t, t): G0[t] for t in types}
    Go, So = orc.dfmf(R, {('b', 'b'): [th]}, types, ranks, max_iter=iters, G0=G0d)
    out, _, _ = fit_owned('dfmf', R, None, {('b', 'b'): [TC.entries_of(th)]}, types, ranks, G0d, iters, size)
    what = 'owned f64 DFMF, constraint as entries%s, %d ranks vs oracle' % (' (denser than n^2/16)' if lengths == DENSE_LENGTHS else '', size)
    for q, (G, S) in enumerate(out):
        for t in types:
            within(relerr(G[t, t], Go[t, t]), 1e-9, '%s: rank %d G_%s' % (what, q, t))
        within(relerr(S['b', 'p'][0], So['b', 'p'][0]), 1e-9, '%s: rank %d S_bp' % (what, q))
    _same_on_every_rank(out, types)


# ---- 6. never expanded ------------------------------------------------------------------------------------------------------
def _banded_entries(n_r, n_c, per_row, rs, values):
    """1 to `per_row` entries a row, strictly ascending columns (the way sparse_owned_cases.never_expanded_plans builds its
    relation): (indptr, indices, values)."""
    step = n_c // per_row
    cols = rs.randint(0, step, (n_r, per_row), dtype=np.int32) + (np.arange(per_row, dtype=np.int32) * step)[None, :]
    keep = rs.rand(n_r, per_row) < 0.73
    keep[:, 0] = True
    indptr = np.zeros(n_r + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    return indptr, cols[keep], values(int(indptr[-1]))


def never_expanded_plans(monkeypatch, iterate=True):
    """20 000 objects with a constraint of about 4 entries a row and one row of 10 000, a 20 000 x 16 000 CSR-fed relation,
    f32, rank 64, 2 owners, the default hub threshold (4096: the long row is cut into 3 segments on the rank that owns it).
    toarray() / mask() raise; a rank's workspace stays below a quarter of the dense f32 constraint (a condition: lists and
    factors of this graph are tens of MB against 1.6 GB) and it keeps count + 1 row pointers."""
    monkeypatch.delenv('SKF_THETA_HUB_ROW', raising=False)
    n_r, n_c, long_row = 20000, 16000, 12345
    rs = np.random.RandomState(0)
    rel = KnownEntries(*_banded_entries(n_r, n_c, 4, rs, lambda k: rs.randint(1, 64, k) / 8.0), shape=(n_r, n_c), unstored='zero')
    ip, ix, vv = _banded_entries(n_r, n_r, 4, rs, lambda k: rs.randint(1, 8, k) / 64.0 * np.where(rs.rand(k) < 0.5, -1.0, 1.0))
    a, b = int(ip[long_row]), int(ip[long_row + 1])
    hub_cols = np.arange(0, n_r, 2, dtype=np.int32)
    hub_vals = rs.randint(1, 8, hub_cols.size) / 64.0 * np.where(rs.rand(hub_cols.size) < 0.5, -1.0, 1.0)
    ix = np.concatenate([ix[:a], hub_cols, ix[b:]])
    vv = np.concatenate([vv[:a], hub_vals, vv[b:]])
    ip = ip.copy()
    ip[long_row + 1:] += hub_cols.size - (b - a)
    theta = KnownEntries(ip, ix, vv, (n_r, n_r), unstored='zero')
    theta.validate()
    assert 70000 <= theta.known <= 80000 and ip[long_row + 1] - ip[long_row] == 10000

    def refuse(*a, **k):
        raise AssertionError('entries were expanded')
    monkeypatch.setattr(KnownEntries, 'toarray', refuse)
    monkeypatch.setattr(KnownEntries, 'mask', refuse)
    types, n, ranks = ['row', 'col'], {'row': n_r, 'col': n_c}, {'row': 64, 'col': 64}
    size = 2
    rt = nat.get_runtime()
    plans = [owned_plan(nat.SKF_DFMF, [('row', 'col', rel, None)], [('row', theta)], types, n, ranks, 'f32', None, q, size)
             for q in range(size)]
    try:
        dense = n_r * n_r * 4
        for q, p in enumerate(plans):
            begin, count, _ = owned_rows('f32', n_r, q, size)
            print('rank %d of %d: workspace %d B, dense f32 constraint %d B' % (q, size, p.workspace_bytes, dense))
            assert p.workspace_bytes < dense // 4, p.workspace_bytes
            rp, ci, _ = p.constraint_lists(0)
            assert rp.shape == (count + 1,) and rp[0] == 0 and rp[-1] == ci.size == ip[begin + count] - ip[begin]
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


# ---- 7. the public API, one process -----------------------------------------------------------------------------------------
def api_case(cls_name, dtype, monkeypatch):
    """Dfmf / Dfmc(shard='owned'), sparse_constraints None and True: the scipy.sparse constraint is never expanded and the
    fit is the fit of the ndarray constraint, bit for bit; False still calls toarray(); shard='relations' still expands."""
    import skfusion_amd.fusion as F
    cls = getattr(F, cls_name)
    coo, dense = TC.api_theta(60, 6)
    assert coo.tocsr().nnz <= 60 * 60 // 16
    args = dict(max_iter=3, init_type='random', random_state=1, dtype=dtype, shard='owned')
    want = cls(**args).fuse(TC.api_graph(dense))
    for sc in (None, True):
        got = cls(sparse_constraints=sc, **args).fuse(TC.api_graph(TC.forbid(monkeypatch, coo.tocsr())))
        TC.same_fits(got, want, "%s %s shard='owned' sparse_constraints=%r" % (cls_name, dtype, sc))
        assert not TC.expanded(TC.api_graph(coo.tocsr()), cls(sparse_constraints=sc, **args))
    calls = []
    sp = coo.tocsr()
    orig = sp.toarray
    monkeypatch.setattr(sp, 'toarray', lambda *a, **k: (calls.append(1), orig(*a, **k))[1], raising=False)
    off = cls(sparse_constraints=False, **args).fuse(TC.api_graph(sp))
    assert calls
    TC.same_fits(off, want, "%s %s shard='owned' sparse_constraints=False" % (cls_name, dtype))
    assert TC.expanded(TC.api_graph(coo.tocsr()), cls(shard='relations', sparse_constraints=True, max_iter=1))
    assert TC.expanded(TC.api_graph(coo.tocsr()), cls(shard='rows', sparse_constraints=True, max_iter=1))


def functional_seam_case():
    """dfmf() / dfmc(): entries in a sharded fit raise ValueError without the keyword; with sparse_constraints=True
    shard='owned' takes them (and gives the fit of the ndarray), 'rows' / 'relations' keep refusing."""
    from skfusion_amd.fusion.decomposition import _dfmf, _dfmc
    rs = np.random.RandomState(0)
    th = 0.05 * np.eye(24)                              # lambda I and three must-link / cannot-link pairs
    for (i, j), v in {(1, 5): -0.125, (2, 9): 0.25, (20, 3): -0.0625}.items():
        th[i, j] = th[j, i] = v
    assert np.count_nonzero(th) <= 24 * 24 // 16        # (the dense-fed plan compacts it to the same lists)
    R = {('a', 'b'): [rs.rand(24, 10)]}
    types, ranks = ['a', 'b'], {'a': 3, 'b': 2}
    G0 = {('a', 'a'): rs.rand(24, 3) + 0.1, ('b', 'b'): rs.rand(10, 2) + 0.1}
    as_entries, as_array = {('a', 'a'): [TC.entries_of(th)]}, {('a', 'a'): [th]}
    fits = {'dfmf': lambda Theta, **kw: _dfmf.dfmf(R, Theta, types, ranks, max_iter=2, G0=G0, **kw),
            'dfmc': lambda Theta, **kw: _dfmc.dfmc(R, {('a', 'b'): [None]}, Theta, types, ranks, max_iter=2, G0=G0, **kw)}
    for name, fit in fits.items():
        for shard in ('relations', 'rows', 'owned'):
            with pytest.raises(ValueError, match='entries'):
                fit(as_entries, shard=shard)
        for shard in ('relations', 'rows'):
            with pytest.raises(ValueError, match='entries'):
                fit(as_entries, shard=shard, sparse_constraints=True)
        Ge, Se = fit(as_entries, shard='owned', sparse_constraints=True)
        Gd, Sd = fit(as_array, shard='owned')
        for k in Gd:
            assert np.array_equal(Ge[k], Gd[k]), (name, k)
        assert np.array_equal(Se['a', 'b'][0], Sd['a', 'b'][0]), name
    mem = nat.get_runtime().mem
    ke = TC.entries_of(th)
    dev = DeviceKnownEntries(mem.from_host(ke.indptr), mem.from_host(ke.indices), mem.from_host(ke.values), ke.shape, ke.known,
                             unstored='zero')
    with pytest.raises(ValueError, match='slices the entries on the host'):      # (as for relations)
        owned_plan(nat.SKF_DFMF, [('a', 'b', R['a', 'b'][0], None)], [('a', dev)], types, {'a': 24, 'b': 10}, ranks, 'f64', None, 0, 1)
