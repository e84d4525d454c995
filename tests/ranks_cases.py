"""Ranks of held-out pairs without the dense reconstruction (csrc/skf_complete.h complete_rank_scores_kernel /
complete_rank_count_kernel, skf_complete_ranks, _engine.DeviceCompleter.ranks, FusionFit.complete_ranks) -- the SAME cases on
the host emulator (small) and on the GPU.  The yardstick is host NumPy in float64; inputs, bound and lists are those of
tests/complete_cases.py.

    rank(r, j) = #{ j' != j admissible for row r (in range, not excluded, score not NaN):
                    score(r, j') > score(r, j)  or  (score(r, j') == score(r, j) and j' < j) },   -1 for a NaN target

  1. exact cases (lattice factors: every partial sum exact): out_rank is the host count index for index, out_val the float64
     score bit for bit, the bytes do not depend on col_splits, and P1 holds against skf_complete_topk: a target that is not
     excluded and has rank p < k sits at slot p of its row's list with the same value bits; with p >= k it is not listed.
  2. random cases: with b = complete_cases.bound (valid for every summation order) a competitor j' certainly beats j when
     X64[r, j'] - X64[r, j] > b[r, j'] + b[r, j] and certainly does not when the difference is < -(b[r, j'] + b[r, j]):
     lo <= rank <= hi with the two counts, |out_val - X64| <= b, and P1 exactly against the device's own top-k.
  3. NaN, 4. refusals with sentinels behind every output, 5. the public API."""
import ctypes as C

import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DeviceCompleter
from complete_cases import Raw, bound, exclusion_mask, host_topk, lattice_factors, lists_of, random_factors

SPLITS = (0, 1, 2, 3, 32)


# ---- targets ----------------------------------------------------------------------------------------------------------------
def target_mask(m, n_cols, seed=0):
    """Boolean [m, n_cols]: row 1 has no target; row 0 and the last row the columns 0, 63, 64 and n_cols - 1 where they
    exist; the last row but one 70 targets when n_cols >= 203 (three chunks of 32, in the second 64-row tile); a random
    handful (0 .. 6) elsewhere -- the rows the 'heavy' pattern excludes entirely or almost entirely among them."""
    rs = np.random.RandomState(seed + 11)
    tg = np.zeros((m, n_cols), dtype=bool)
    for r in range(m):
        tg[r, rs.choice(n_cols, size=min(rs.randint(0, 7), n_cols), replace=False)] = True
    for r in (0, m - 1):
        for j in (0, 63, 64, n_cols - 1):
            if 0 <= j < n_cols:
                tg[r, j] = True
    if n_cols >= 203:
        tg[m - 3, :] = False
        tg[m - 3, rs.choice(n_cols, size=70, replace=False)] = True
    tg[1 % m, :] = False
    return tg


# ---- the host's answer ------------------------------------------------------------------------------------------------------
def host_ranks(X, tlists, ex=None):
    """The definition, target by target, on the float64 scores X."""
    indptr, indices = tlists
    out = np.empty(len(indices), dtype=np.int64)
    cols = np.arange(X.shape[1])
    for r in range(X.shape[0]):
        ok = ~np.isnan(X[r])
        if ex is not None:
            ok &= ~ex[r]
        for e in range(indptr[r], indptr[r + 1]):
            j, s = indices[e], X[r, indices[e]]
            out[e] = -1 if np.isnan(s) else int((ok & ((X[r] > s) | ((X[r] == s) & (cols < j)))).sum())
    return out


def rank_interval(X64, B, tlists, ex=None):
    """(lo, hi) of the random cases: the competitors that beat the target by more than both bounds / that are not beaten
    by more than both bounds."""
    indptr, indices = tlists
    lo = np.empty(len(indices), dtype=np.int64)
    hi = np.empty(len(indices), dtype=np.int64)
    for r in range(X64.shape[0]):
        ok = np.ones(X64.shape[1], dtype=bool) if ex is None else ~ex[r]
        for e in range(indptr[r], indptr[r + 1]):
            j = indices[e]
            others = ok.copy()
            others[j] = False
            d, tol = X64[r] - X64[r, j], B[r] + B[r, j]
            lo[e] = int((others & (d > tol)).sum())
            hi[e] = int((others & (d >= -tol)).sum())
    return lo, hi


def rows_of(tlists):
    return np.repeat(np.arange(len(tlists[0]) - 1), np.diff(tlists[0]))


def check_p1(rank, val, tlists, ex, idx, tval, k, what):
    """P1 against a top-k result (idx, tval) of the same inputs; `val` None: indices only."""
    rows, cols = rows_of(tlists), tlists[1]
    for e in range(len(cols)):
        r, j, p = rows[e], cols[e], rank[e]
        if p < 0 or (ex is not None and ex[r, j]):
            continue
        if p < k:
            assert idx[r, p] == j, '%s: target (%d, %d) has rank %d, slot holds column %d' % (what, r, j, p, idx[r, p])
            if val is not None:
                assert np.array_equal(tval[r, p:p + 1], val[e:e + 1]), '%s: target (%d, %d): value bits differ' % (what, r, j)
        else:
            assert j not in idx[r], '%s: target (%d, %d) has rank %d and is listed' % (what, r, j, p)


# ---- the C ABI, called directly ----------------------------------------------------------------------------------------------
def raw_workspace(raw, n, col_splits=0):
    need = C.c_size_t()
    raw.rt.call('skf_complete_ranks_workspace_bytes', raw.code, raw.m, raw.n_cols, n, col_splits, C.byref(need))
    return need.value


def raw_ranks(raw, tlists, ex=None, col_splits=0, xlists=None, status=False, n_targets=None, keep_val=True):
    """skf_complete_ranks on the buffers of a complete_cases.Raw, sentinels behind both outputs."""
    rt, mem = raw.rt, raw.rt.mem
    tp, ti = np.asarray(tlists[0], dtype=np.int64), np.asarray(tlists[1], dtype=np.int32)
    n = len(ti) if n_targets is None else n_targets
    size = max(n, len(ti)) + 1
    orank = mem.from_host(np.full(size, -7, dtype=np.int32))
    oval = mem.from_host(np.full(size, -7.0, dtype=raw.T))
    ws = mem.empty(raw_workspace(raw, n, col_splits))
    btp, bti = mem.from_host(tp), mem.from_host(ti if len(ti) else np.zeros(1, dtype=np.int32))
    xp = xi = None
    if xlists is None and ex is not None:
        xlists = lists_of(ex)
    if xlists is not None:
        xp = mem.from_host(np.asarray(xlists[0], dtype=np.int64))
        xi = mem.from_host(np.asarray(xlists[1], dtype=np.int32) if len(xlists[1]) else np.zeros(1, dtype=np.int32))
    rc = rt.lib.skf_complete_ranks(raw.code, raw.h.ptr, raw.ldh, raw.m, raw.g.ptr, raw.ldg, raw.n_cols, raw.c, btp.ptr, bti.ptr, n,
                                   xp.ptr if xp else None, xi.ptr if xi else None, orank.ptr, oval.ptr if keep_val else None,
                                   col_splits, ws.ptr, ws.nbytes, mem.stream)
    mem.synchronize()
    gr, gv = mem.to_host(orank, (size,), np.int32), mem.to_host(oval, (size,), raw.T)
    if status:
        return rc, gr, gv
    rt.check(rc)
    assert (gr[n:] == -7).all() and (gv[n:] == -7.0).all(), 'memory behind target n changed'
    if not keep_val:
        assert (gv == -7.0).all(), 'out_val was NULL and the buffer next to it changed'
    return gr[:n].copy(), gv[:n].copy()


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------
def exact_case(dtype, m, n_cols, ranks, patterns=('none', 'edges', 'heavy'), splits=SPLITS):
    G_row, S, G_col = lattice_factors(m, n_cols, ranks)
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    assert X.max() * 512 < 2 ** 23 and np.array_equal(X.astype(np.float32).astype(np.float64), X)      # exact in f32
    raw = Raw(dtype, H, G_col)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    tg = target_mask(m, n_cols)
    tl = lists_of(tg)
    rows = rows_of(tl)
    k = min(64, n_cols)
    if n_cols >= 203:
        assert np.diff(tl[0]).max() == 70 and (np.diff(tl[0]) == 0).any()
    for pattern in patterns:
        ex = exclusion_mask(pattern, m, n_cols)
        what = 'ranks exact %s m %d n %d ranks %r %s' % (dtype, m, n_cols, ranks, pattern)
        want = host_ranks(X, tl, ex)
        if ex is not None:
            assert ex[rows, tl[1]].any(), 'no target is itself excluded'
        first = None
        for s in splits:
            gr, gv = raw_ranks(raw, tl, ex, col_splits=s)
            assert np.array_equal(gr, want), '%s splits %d: ranks differ from the host count' % (what, s)
            assert np.array_equal(gv.astype(np.float64), X[rows, tl[1]]), '%s splits %d: values differ from the host scores' % (what, s)
            if first is None:
                first = (gr.tobytes(), gv.tobytes())
            assert (gr.tobytes(), gv.tobytes()) == first, '%s: col_splits %d changes the bytes' % (what, s)
        ti, tv = host_topk(X, k, ex)
        check_p1(want, None, tl, ex, ti, tv, k, what + ' P1 of the host order')
        gr, gv = raw_ranks(raw, tl, ex)
        for s in (0, 3):
            ti, tv = raw.topk(k, ex, col_splits=s)
            check_p1(gr, gv, tl, ex, ti, tv, k, '%s P1 top-k splits %d' % (what, s))
        # out_val NULL: the scores live in the workspace, the ranks are the same
        g2, _ = raw_ranks(raw, tl, ex, keep_val=False)
        assert np.array_equal(g2, want), what + ': out_val NULL'
        # the engine path (H by skf_gemm)
        er, ev = comp.ranks(G_row, tl, exclude=None if ex is None else lists_of(ex))
        assert er.dtype == np.int32 and ev.dtype == np.float64
        assert np.array_equal(er, want) and np.array_equal(ev, X[rows, tl[1]]), 'DeviceCompleter.ranks %s' % what
    # no target at all: success, nothing launched, nothing written
    none = (np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    gr, gv = raw_ranks(raw, none)
    assert gr.size == 0
    assert comp.ranks(G_row, none)[0].shape == (0,)


# ---- 2. random cases -------------------------------------------------------------------------------------------------------
def check_random(rank, val, tlists, X64, B, ex, what):
    rows, cols = rows_of(tlists), tlists[1]
    lo, hi = rank_interval(X64, B, tlists, ex)
    bad = np.nonzero((rank < lo) | (rank > hi))[0]
    assert bad.size == 0, '%s: target %d has rank %d outside [%d, %d]' % (what, bad[0], rank[bad[0]], lo[bad[0]], hi[bad[0]])
    ratio = float((np.abs(val - X64[rows, cols]) / B[rows, cols]).max()) if len(cols) else 0.0
    print('%s: max |out_val - X64| / b = %.3g, widest interval %d' % (what, ratio, int((hi - lo).max()) if len(cols) else 0))
    assert ratio <= 1.0, '%s: a value is %.3e x its bound away' % (what, ratio)
    return ratio


def random_case(dtype, ranks, m=131, n_cols=997, pattern='edges', label=''):
    G_row, S, G_col = random_factors(m, n_cols, ranks)
    X64 = np.dot(np.dot(G_row, S), G_col.T)
    B = bound(G_row, S, G_col, dtype)
    ex = exclusion_mask(pattern, m, n_cols)
    xl = None if ex is None else lists_of(ex)
    tl = lists_of(target_mask(m, n_cols))
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    what = '%s ranks random %s ranks %r %s' % (label, dtype, ranks, pattern)
    rank, val = comp.ranks(G_row, tl, exclude=xl)
    check_random(rank, val, tl, X64, B, ex, what)
    for s in (1, 3, 32):
        r2, v2 = comp.ranks(G_row, tl, exclude=xl, col_splits=s)
        assert rank.tobytes() == r2.tobytes() and val.tobytes() == v2.tobytes(), what + ': col_splits %d changes the bytes' % s
    idx, tval = comp.topk(G_row, 64, exclude=xl)
    check_p1(rank, val, tl, ex, idx, tval, 64, what + ' P1')
    return rank, val


# ---- 3. NaN -----------------------------------------------------------------------------------------------------------------
def nan_case(dtype, m=67, n_cols=203, ranks=(5, 7)):
    G_row, S, G_col = lattice_factors(m, n_cols, ranks)
    H = np.dot(G_row, S)
    tg = target_mask(m, n_cols)
    rn, jn = 9, 70
    tg[rn, [2, 100]] = True
    tg[[4, 66], jn] = True
    tl = lists_of(tg)
    rows = rows_of(tl)
    ex = exclusion_mask('edges', m, n_cols)
    clean, _ = raw_ranks(Raw(dtype, H, G_col), tl, ex)
    # a NaN row of H: all its targets get -1, nobody else notices
    Hn = H.copy()
    Hn[rn, 1] = np.nan
    gr, gv = raw_ranks(Raw(dtype, Hn, G_col), tl, ex)
    assert (gr[rows == rn] == -1).all() and np.isnan(gv[rows == rn]).all() and (rows == rn).sum() >= 2
    assert np.array_equal(gr[rows != rn], clean[rows != rn])
    # a NaN row of Gc: that column is never counted and a target on it gets -1; every other rank is the one of the run
    # with that column excluded in every row
    Gn = G_col.copy()
    Gn[jn, 0] = np.nan
    Xn = np.dot(H, Gn.T)
    gr, gv = raw_ranks(Raw(dtype, H, Gn), tl, ex)
    on = tl[1] == jn
    assert on.sum() >= 2 and (gr[on] == -1).all() and np.isnan(gv[on]).all()
    assert np.array_equal(gr, host_ranks(Xn, tl, ex))
    ex2 = ex.copy()
    ex2[:, jn] = True
    without, _ = raw_ranks(Raw(dtype, H, G_col), tl, ex2)
    assert np.array_equal(gr[~on], without[~on]) and (gr[~on] >= 0).all()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def refusals_without_device(lib, ptr):
    """Everything refused before any launch (`ptr`: any non-null, 256-byte aligned address; it is never dereferenced)."""
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    need = C.c_size_t()
    assert lib.skf_complete_ranks_workspace_bytes(nat.SKF_F32, 67, 203, 100, 0, C.byref(need)) == 0 and need.value >= 512 + 400
    nb = need.value
    assert nb < 4096, 'the workspace holds flag words and one score per target, nothing of the size of the relation'

    def ranks(dtype=nat.SKF_F32, H=ptr, Gc=ptr, c=8, tp=ptr, ti=ptr, n=100, xp=None, xi=None, orank=ptr, oval=ptr, ws=ptr, ws_bytes=nb,
              splits=0, m=67):
        return lib.skf_complete_ranks(dtype, H, c, m, Gc, c, 203, c, tp, ti, n, xp, xi, orank, oval, splits, ws, ws_bytes, None)
    for kw in (dict(c=0), dict(c=1025), dict(H=None), dict(Gc=None), dict(orank=None), dict(tp=None), dict(ti=None), dict(xp=ptr),
               dict(xi=ptr), dict(dtype=nat.SKF_BF16), dict(splits=-1), dict(splits=33), dict(m=2 ** 31), dict(n=-1)):
        assert ranks(**kw) == INV, kw
        assert b'skf_complete_ranks' in lib.skf_last_error()
    assert ranks(ws_bytes=nb - 1) == WS and ranks(ws=None) == WS
    assert ranks(n=0, tp=ptr, ti=ptr) == 0                       # no target: success without a launch
    for kw in (dict(splits=33), dict(m=-1), dict(n=-1), dict(dtype=nat.SKF_BF16)):
        assert lib.skf_complete_ranks_workspace_bytes(kw.get('dtype', nat.SKF_F32), kw.get('m', 67), 203, kw.get('n', 100),
                                                      kw.get('splits', 0), C.byref(need)) == INV, kw
    assert lib.skf_complete_ranks_workspace_bytes(nat.SKF_F32, 67, 203, 100, 0, None) == INV
    for s in (0, 1, 32):
        assert lib.skf_complete_ranks_workspace_bytes(nat.SKF_F64, 67, 203, 100, s, C.byref(need)) == 0
        assert need.value >= 512 + 800 and ranks(dtype=nat.SKF_F64, splits=s, ws_bytes=need.value - 1) == WS, s


def defective_lists(p, i, m, n_cols):
    """name -> (indptr, indices, count handed over): every defect of a CSR list the header names."""
    a, b = int(p[4]), int(p[5])
    assert b - a >= 2
    bad = {}
    j = i.copy(); j[a], j[a + 1] = i[a + 1], i[a]; bad['descending'] = (p, j, len(i))
    j = i.copy(); j[a] = j[a + 1]; bad['repeated'] = (p, j, len(i))
    j = i.copy(); j[b - 1] = n_cols; bad['column past the end'] = (p, j, len(i))
    j = i.copy(); j[a] = -1; bad['negative column'] = (p, j, len(i))
    q = p.copy(); q[0] = 1; bad['indptr does not start at 0'] = (q, i, len(i))
    q = p.copy(); q[5] = p[4] - 1; bad['indptr decreases'] = (q, i, len(i))
    q = p.copy(); q[m] = p[m] - 1; bad['indptr does not end at its count'] = (q, i, len(i))
    q = p.copy(); q[m] = p[m - 1] - 1; bad['indptr falls at its end'] = (q, i, len(i))
    q = p.copy(); q[m] = -3; bad['negative count'] = (q, i, len(i))
    bad['count does not match indptr[m]'] = (p, i, len(i) - 1)
    q = p.copy(); q[7] = p[m] + 5; bad['indptr past the count'] = (q, i, len(i))
    return bad


def refusals_case(dtype='f64'):
    rt = nat.get_runtime()
    keep = rt.mem.empty(4096)
    refusals_without_device(rt.lib, keep.ptr)
    m, n_cols = 37, 70
    G_row, S, G_col = lattice_factors(m, n_cols, (5, 7))
    raw = Raw(dtype, np.dot(G_row, S), G_col)
    ex = exclusion_mask('edges', m, n_cols)
    xl = lists_of(ex)
    tg = target_mask(m, n_cols)
    tg[4, :5] = True
    tl = lists_of(tg)
    for name, (p, i, n) in defective_lists(tl[0], tl[1], m, n_cols).items():
        for s in (1, 2):
            rc, gr, gv = raw_ranks(raw, (p, i), xlists=xl, col_splits=s, status=True, n_targets=n)
            assert rc == nat.SKF_E_INVALID and b'target lists' in rt.lib.skf_last_error(), 'targets: ' + name
            assert (gr == -7).all() and (gv == -7.0).all(), 'targets: %s: outputs were written' % name
    for name, (p, i, n) in defective_lists(xl[0], xl[1], m, n_cols).items():
        if name in ('count does not match indptr[m]', 'indptr does not end at its count'):
            continue                                             # (the exclusion lists carry no count but indptr[m])
        rc, gr, gv = raw_ranks(raw, tl, xlists=(p, i), status=True)
        assert rc == nat.SKF_E_INVALID and b'exclusion lists' in rt.lib.skf_last_error(), 'exclusion: ' + name
        assert (gr == -7).all() and (gv == -7.0).all(), 'exclusion: %s: outputs were written' % name
    # a workspace one byte short, on real buffers
    mem = rt.mem
    n = len(tl[1])
    orank, ws = mem.from_host(np.full(n, -7, dtype=np.int32)), mem.empty(raw_workspace(raw, n))
    tp, ti = mem.from_host(tl[0]), mem.from_host(tl[1])
    rc = rt.lib.skf_complete_ranks(raw.code, raw.h.ptr, raw.ldh, m, raw.g.ptr, raw.ldg, n_cols, raw.c, tp.ptr, ti.ptr, n, None, None,
                                   orank.ptr, None, 0, ws.ptr, ws.nbytes - 1, mem.stream)
    mem.synchronize()
    assert rc == nat.SKF_E_WORKSPACE and (mem.to_host(orank, (n,), np.int32) == -7).all()
    gr, _ = raw_ranks(raw, tl, ex)                               # and the lists as they were are accepted
    assert np.array_equal(gr, host_ranks(np.dot(np.dot(G_row, S), G_col.T), tl, ex))


# ---- 5. public API ----------------------------------------------------------------------------------------------------------
def api_case(kind, dtype, monkeypatch):
    """kind 'dfmc-masked': Dfmc on a MaskedArray relation; 'dfmf-csr': Dfmf on a scipy.sparse relation (40 x 30, ranks 5 / 4)."""
    import scipy.sparse
    import known_csr_api_cases as KA
    from skfusion_amd.fusion import Dfmc, Dfmf, Relation, ObjectType
    from skfusion_amd.fusion.base import DataFusionError
    csr, ma = KA.ratings(40, 30, 0.2, 11)
    sparse = kind == 'dfmf-csr'
    g, users, movies = KA.graph(csr if sparse else ma, ranks=(5, 4, 3))
    fuser = KA.fit(Dfmf if sparse else Dfmc, g, max_iter=5, init_type='random', random_state=0, dtype=dtype)
    rel = list(g.relations)[0]
    known = ~np.ma.getmaskarray(ma)
    if sparse:                    # from here on nothing may expand a sparse matrix
        def boom(*a, **kw):
            raise AssertionError('a sparse matrix was densified')
        for cls in (scipy.sparse.csr_matrix, scipy.sparse.csc_matrix, scipy.sparse.coo_matrix):
            monkeypatch.setattr(cls, 'toarray', boom)
            monkeypatch.setattr(cls, 'todense', boom)
    X = fuser.complete(rel)
    B = bound(fuser.factor(users), fuser.backbone(rel), fuser.factor(movies), dtype)
    what = 'api ranks %s %s' % (kind, dtype)
    rs = np.random.RandomState(4)
    rows, cols = rs.randint(0, 40, 200), rs.randint(0, 30, 200)
    rows[150:], cols[150:] = rows[:50], cols[:50]                 # duplicates
    order = rs.permutation(200)
    rows, cols = rows[order], cols[order]
    assert np.unique(rows * 30 + cols).size < 200 and (np.diff(rows) < 0).any()
    rank = fuser.complete_ranks(rel, rows, cols, exclude='known', dtype=dtype)
    assert rank.dtype == np.int64 and rank.shape == (200,)
    for e in range(200):          # the interval of the random cases, pair by pair
        r, j = rows[e], cols[e]
        others = ~known[r]
        others[j] = False
        d, tol = X[r] - X[r, j], B[r] + B[r, j]
        lo, hi = int((others & (d > tol)).sum()), int((others & (d >= -tol)).sum())
        assert lo <= rank[e] <= hi, '%s: pair (%d, %d) has rank %d outside [%d, %d]' % (what, r, j, rank[e], lo, hi)
    idx, _ = fuser.complete_topk(rel, 5, exclude='known', dtype=dtype)
    for e in range(200):          # P1
        r, j = rows[e], cols[e]
        if known[r, j]:
            continue
        if rank[e] < 5:
            assert idx[r, rank[e]] == j, '%s: P1 at pair (%d, %d)' % (what, r, j)
        else:
            assert j not in idx[r], '%s: P1 at pair (%d, %d)' % (what, r, j)
    assert np.array_equal(fuser.complete_ranks(rel, rows, cols, exclude='known', dtype=dtype, block_rows=2), rank), what + ': block_rows'
    pat = scipy.sparse.csr_matrix((np.ones(int(known.sum())), np.nonzero(known)), shape=known.shape)
    for fmt in (pat, pat.tocsc(), pat.tocoo()):
        assert np.array_equal(fuser.complete_ranks(rel, rows, cols, exclude=fmt, dtype=dtype), rank), what + ': exclude= as %s' % fmt.format
    free = fuser.complete_ranks(rel, rows, cols, dtype=dtype)
    assert (free >= rank).all() and (free > rank).any(), what + ': no exclusion cannot rank a pair better'
    assert fuser.complete_ranks(rel, np.zeros(0, dtype=int), np.zeros(0, dtype=int), dtype=dtype).shape == (0,)
    # refusals
    with pytest.raises(DataFusionError, match='shape'):
        fuser.complete_ranks(rel, rows, cols, exclude=pat[:, :20], dtype=dtype)
    with pytest.raises(DataFusionError):
        fuser.complete_ranks(rel, [40], [0], dtype=dtype)
    with pytest.raises(DataFusionError):
        fuser.complete_ranks(rel, [0], [30], dtype=dtype)
    with pytest.raises(DataFusionError):
        fuser.complete_ranks(rel, [-1], [0], dtype=dtype)
    with pytest.raises(DataFusionError):
        fuser.complete_ranks(rel, [0, 1], [0], dtype=dtype)
    plain = list(g.relations)[1]                                 # movies x genres: a plain ndarray
    with pytest.raises(DataFusionError, match='plain array'):
        fuser.complete_ranks(plain, [0], [0], exclude='known', dtype=dtype)
    stranger = Relation(np.zeros((40, 3)), users, ObjectType('strangers', 2))
    with pytest.raises(DataFusionError):
        fuser.complete_ranks(stranger, [0], [0], dtype=dtype)
    post = Relation(rel.data, users, movies, postprocessor=lambda x: np.clip(x, 0.0, 1.0), **({} if not sparse else {'unstored': rel.unstored}))
    fuser.backbones_[post] = fuser.backbones_[rel]
    with pytest.raises(DataFusionError, match='postprocessor'):
        fuser.complete_ranks(post, [0], [0], dtype=dtype)
    return fuser


def api_runs_case(dtype='f64'):
    """n_run = 2 and run=None: a generator over the runs, each equal to the explicit run."""
    import types
    import known_csr_api_cases as KA
    from skfusion_amd.fusion import Dfmc
    _, ma = KA.ratings(40, 30, 0.2, 11)
    g, users, movies = KA.graph(ma, ranks=(5, 4, 3))
    fuser = KA.fit(Dfmc, g, max_iter=3, init_type='random', random_state=0, dtype=dtype, n_run=2)
    rel = list(g.relations)[0]
    rs = np.random.RandomState(6)
    rows, cols = rs.randint(0, 40, 60), rs.randint(0, 30, 60)
    rk = fuser.complete_ranks(rel, rows, cols, exclude='known', dtype=dtype)
    assert isinstance(rk, types.GeneratorType)
    rk = list(rk)
    assert len(rk) == 2
    for r in range(2):
        assert np.array_equal(rk[r], fuser.complete_ranks(rel, rows, cols, exclude='known', run=r, dtype=dtype))
    assert not np.array_equal(rk[0], rk[1])
