"""Every pair at or above a per-row threshold as CSR, without the dense reconstruction (csrc/skf_complete.h
complete_above_kernel and the scan kernels, skf_complete_above, _engine.DeviceCompleter.above, FusionFit.complete_above) --
the SAME cases on the host emulator (small) and on the GPU.  The yardstick is host NumPy in float64; inputs, bound and lists
are those of tests/complete_cases.py.

    above(r) = { j in [0, n_cols) : j not excluded for row r, score(r, j) >= thr[r] }     (IEEE: NaN selects nothing)

  1. exact cases (lattice factors: every partial sum exact): out_indptr / out_indices / out_values are the host's
     ok & (X >= thr) index for index and bit for bit, whatever col_splits; count-only, out_values NULL, a capacity one short.
  2. agreement with the operators that exist: P2 against skf_complete_topk (thr = its k-th value: the first k entries of a
     row in top-k order ARE top-k's, every further one equals thr) and against skf_complete_ranks (a target is present exactly
     when its score passes, with the same bits, and the entries ahead of it are as many as its rank).
  3. random cases: with b = complete_cases.bound every admissible pair more than b above its threshold is present, every
     pair more than b below is absent, every value is within b; the pairs within b of the threshold are undecided and must be
     at most 0.1 % of all pairs (measured on the host with the reference arithmetic: 0 of 13 601 at 67 x 203; at 131 x 997
     ranks (20, 64) 10 of 130 607 in f32 and 0 in f64; 0 at ranks (5, 7)).
  4. NaN, 5. refusals with sentinels behind every output, 6. the public API."""
import ctypes as C

import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DeviceCompleter
from complete_cases import Raw, bound, exclusion_mask, host_topk, lattice_factors, lists_of, random_factors
from ranks_cases import host_ranks, raw_ranks, rows_of, target_mask

SPLITS = (0, 1, 2, 3, 32)
PAD = 5                                          # sentinel entries behind every output


# ---- the host's answer ------------------------------------------------------------------------------------------------------
def host_above(X, thr, ex=None):
    """(indptr, indices, values) of ok & (X >= thr) on the float64 scores X; a NaN on either side compares false."""
    with np.errstate(invalid='ignore'):
        sel = X >= np.asarray(thr, dtype=np.float64)[:, None]
    if ex is not None:
        sel &= ~ex
    indptr = np.zeros(X.shape[0] + 1, dtype=np.int64)
    np.cumsum(sel.sum(axis=1), out=indptr[1:])
    return indptr, np.nonzero(sel)[1].astype(np.int32), X[sel]


def own_thresholds(X, seed=0):
    """Per row a score of the row itself (so that the tie at the threshold is selected); rows 2, 5, 6 and 8 (where they
    exist) get -inf, +inf, NaN and a value above the row's maximum."""
    m, n = X.shape
    rs = np.random.RandomState(seed + 3)
    thr = X[np.arange(m), rs.randint(0, n, size=m)].copy()
    for r, v in ((2, -np.inf), (5, np.inf), (6, np.nan)):
        if r < m:
            thr[r] = v
    if 8 < m:
        thr[8] = X[8].max() + 1.0
    return thr


# ---- the C ABI, called directly ----------------------------------------------------------------------------------------------
def raw_workspace(raw, col_splits=0, m=None):
    need = C.c_size_t()
    raw.rt.call('skf_complete_above_workspace_bytes', raw.code, raw.m if m is None else m, raw.n_cols, col_splits, C.byref(need))
    return need.value


def call_above(raw, thr_host, xlists=None, col_splits=0, capacity=None, **over):
    """skf_complete_above on the buffers of a complete_cases.Raw with sentinels in and behind every output.  `over` replaces
    single arguments (None: a NULL pointer).  Returns (status, indptr [m + 1 + PAD], indices [capacity + PAD], values
    [capacity + PAD], n_found) as they stand after the call, and the capacity handed over."""
    rt, mem = raw.rt, raw.rt.mem
    m = raw.m
    cap = m * raw.n_cols if capacity is None else capacity
    bt = mem.from_host(np.asarray(thr_host, dtype=raw.T) if m else np.zeros(1, dtype=raw.T))
    optr = mem.from_host(np.full(m + 1 + PAD, -7, dtype=np.int64))
    oidx = mem.from_host(np.full(cap + PAD, -7, dtype=np.int32))
    oval = mem.from_host(np.full(cap + PAD, -7.0, dtype=raw.T))
    ws = mem.empty(raw_workspace(raw, col_splits))      # exactly what the query asks for
    xp = xi = None
    if xlists is not None:
        xp = mem.from_host(np.asarray(xlists[0], dtype=np.int64))
        xi = mem.from_host(np.asarray(xlists[1], dtype=np.int32) if len(xlists[1]) else np.zeros(1, dtype=np.int32))
    found = C.c_int64(-7)
    a = dict(dtype=raw.code, H=raw.h.ptr, ldh=raw.ldh, m=m, Gc=raw.g.ptr, ldg=raw.ldg, n_cols=raw.n_cols, c=raw.c, thr=bt.ptr,
             xp=xp.ptr if xp else None, xi=xi.ptr if xi else None, cap=cap, optr=optr.ptr, oidx=oidx.ptr, oval=oval.ptr,
             found=C.byref(found), splits=col_splits, ws=ws.ptr, ws_bytes=ws.nbytes)
    assert set(over) <= set(a), over
    a.update(over)
    rc = rt.lib.skf_complete_above(a['dtype'], a['H'], a['ldh'], a['m'], a['Gc'], a['ldg'], a['n_cols'], a['c'], a['thr'], a['xp'],
                                   a['xi'], a['cap'], a['optr'], a['oidx'], a['oval'], a['found'], a['splits'], a['ws'],
                                   a['ws_bytes'], mem.stream)
    mem.synchronize()
    return (rc, mem.to_host(optr, (m + 1 + PAD,), np.int64), mem.to_host(oidx, (cap + PAD,), np.int32),
            mem.to_host(oval, (cap + PAD,), raw.T), found.value), cap


def untouched(res):
    rc, p, i, v, n = res
    return (p == -7).all() and (i == -7).all() and (v == -7.0).all() and n == -7


def raw_above(raw, thr, ex=None, col_splits=0, xlists=None, capacity=None, mode='full'):
    """A successful call: (indptr, indices, values) cut to size; the memory behind entry n_found must be as it was.
    mode 'pattern': out_values NULL; 'count': out_indices NULL too."""
    if xlists is None and ex is not None:
        xlists = lists_of(ex)
    over = {}
    if mode != 'full':
        over['oval'] = None
    if mode == 'count':
        over['oidx'] = None
    (rc, p, i, v, n), cap = call_above(raw, thr, xlists, col_splits, capacity, **over)
    raw.rt.check(rc)
    m = raw.m
    assert (p[m + 1:] == -7).all(), 'memory behind out_indptr[m] changed'
    assert p[0] == 0 and p[m] == n and (np.diff(p[:m + 1]) >= 0).all(), 'out_indptr is no prefix sum ending at n_found'
    if mode == 'count':
        assert (i == -7).all() and (v == -7.0).all(), 'count only and an entry buffer changed'
        return p[:m + 1].copy(), None, None
    assert n <= cap and (i[n:] == -7).all() and (v[n:] == -7.0).all(), 'memory behind entry n_found changed'
    if mode == 'pattern':
        assert (v == -7.0).all(), 'out_values was NULL and the buffer next to it changed'
        return p[:m + 1].copy(), i[:n].copy(), None
    return p[:m + 1].copy(), i[:n].copy(), v[:n].copy()


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ': out_indptr differs from the host'
    assert np.array_equal(got[1], want[1]), what + ': out_indices differ from the host'
    if got[2] is not None:
        assert np.array_equal(got[2].astype(np.float64), want[2]), what + ': out_values differ from the host scores'


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------
def exact_case(dtype, m, n_cols, ranks, patterns=('none', 'empty', 'edges', 'heavy'), splits=SPLITS):
    G_row, S, G_col = lattice_factors(m, n_cols, ranks)
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    assert X.max() * 512 < 2 ** 23 and np.array_equal(X.astype(np.float32).astype(np.float64), X)      # exact in f32
    raw = Raw(dtype, H, G_col)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    thr = own_thresholds(X)
    ties = 0
    for pattern in patterns:
        ex = exclusion_mask(pattern, m, n_cols)
        what = 'above exact %s m %d n %d ranks %r %s' % (dtype, m, n_cols, ranks, pattern)
        want = host_above(X, thr, ex)
        total = int(want[0][-1])
        ok = np.ones_like(X, dtype=bool) if ex is None else ~ex
        ties += int((ok & (X == thr[:, None])).sum())
        for r in (2, 5, 6, 8):                                       # -inf: everything admissible; +inf, NaN, above the maximum: nothing
            assert want[0][r + 1] - want[0][r] == (int(ok[r].sum()) if r == 2 else 0)
        first = None
        for s in splits:
            got = raw_above(raw, thr, ex, col_splits=s)
            same(got, want, '%s splits %d' % (what, s))
            b = tuple(x.tobytes() for x in got)
            first = first or b
            assert b == first, '%s: col_splits %d changes the bytes' % (what, s)
        same(raw_above(raw, thr, ex, mode='pattern'), want, what + ' out_values NULL')
        cnt = raw_above(raw, thr, ex, mode='count', col_splits=3)
        assert np.array_equal(cnt[0], want[0]), what + ': count-only indptr'
        same(raw_above(raw, thr, ex, capacity=total), want, what + ' exact capacity')
        if total:
            res, _ = call_above(raw, thr, None if ex is None else lists_of(ex), capacity=total - 1)
            rc, p, i, v, n = res
            msg = raw.rt.lib.skf_last_error()
            assert rc == nat.SKF_E_WORKSPACE and str(total).encode() in msg and str(total - 1).encode() in msg, what + ': %r' % msg
            assert n == total and np.array_equal(p[:m + 1], want[0]) and (p[m + 1:] == -7).all(), what + ': capacity one short'
            assert (i == -7).all() and (v == -7.0).all(), what + ': capacity one short and an entry buffer was written'
        # the engine path (H by skf_gemm): the default capacity and one that forces the repeat give the same arrays
        xl = None if ex is None else lists_of(ex)
        e1 = comp.above(G_row, thr, exclude=xl)
        assert e1[0].dtype == np.int64 and e1[1].dtype == np.int32 and e1[2].dtype == np.float64
        same(e1, want, 'DeviceCompleter.above ' + what)
        e2 = comp.above(G_row, thr, exclude=xl, capacity=max(total // 2, 0), col_splits=2)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(e1, e2)), what + ': the repeat with the exact count differs'
    assert ties > m // 2, 'the tie at the threshold is not exercised'
    # a scalar threshold through the engine
    t0 = float(np.median(X))
    same(comp.above(G_row, t0), host_above(X, np.full(m, t0)), 'DeviceCompleter.above scalar threshold')
    # no row / no column: success, every pointer zero
    empty = Raw(dtype, H[:0], G_col)
    p, i, v = raw_above(empty, np.zeros(0), capacity=0)
    assert p.tolist() == [0] and i.size == 0
    nocol = Raw(dtype, H, G_col[:0])
    p, i, v = raw_above(nocol, thr, capacity=0)
    assert (p == 0).all() and p.shape == (m + 1,) and i.size == 0
    p, i, v = comp.above(G_row[:0], np.zeros(0))
    assert p.tolist() == [0] and i.shape == (0,) and v.shape == (0,)


def scan_case(dtype, m, n_cols=70, ranks=(5, 1), col_splits=2):
    """More rows than one workgroup of the scan holds (256; beyond 262 144 rows a workgroup walks several times): the
    pointers and the (row, split) starts across chunk boundaries.  Rows 64 .. 191 select nothing, so two row tiles of
    the fill pass leave before their first product."""
    G_row, S, G_col = lattice_factors(m, n_cols, ranks)
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    raw = Raw(dtype, H, G_col)
    thr = own_thresholds(X)
    thr[64:192] = np.inf
    ex = exclusion_mask('edges', m, n_cols)
    want = host_above(X, thr, ex)
    assert (np.diff(want[0])[256:] > 0).any() and (np.diff(want[0])[64:192] == 0).all()
    xl = lists_of(ex)
    same(raw_above(raw, thr, xlists=xl, col_splits=col_splits, capacity=int(want[0][-1])), want,
         'above scan %s m %d splits %d' % (dtype, m, col_splits))


def seam_mask(m, n_cols, seam, seed=0):
    """Excluded pairs around `seam`, the first column of a later split: row r lists columns seam - 1 and seam (r % 4 == 0),
    only seam - 1 (1), only seam (2) or neither (3), over a thin random pattern elsewhere, so that the lower bound of the
    later split lands inside a list; row 5's list begins at seam - 1 and row 8's ends at seam."""
    ex = np.random.RandomState(seed + 13).rand(m, n_cols) < 0.0625
    r = np.arange(m)
    ex[:, seam - 1] = r % 4 <= 1
    ex[:, seam] = r % 2 == 0
    ex[5 % m, :seam - 1] = False
    ex[8 % m, seam + 1:] = False
    return ex


def seam_case(dtype, m=67, n_cols=203, ranks=(5, 7), k=10):
    """The first column of the second of two splits (four column tiles, two per split: column 128) against exclusion lists
    that hold columns 127 and 128, one of them or neither, the last (partial) row tile included: top-k, ranks and above bit
    for bit against the host and against the same call with one split."""
    seam = 2 * 64
    assert 3 * 64 < n_cols <= 4 * 64 and m > 64
    # seed 1: columns 127 and 128 are among the ten best of 39 rows on the host (seed 0: of none), so that an entry lost at
    # the seam shows in top-k too; the three asserts on `open_seam` below hold every operator to that
    G_row, S, G_col = lattice_factors(m, n_cols, ranks, seed=1)
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    assert X.max() * 512 < 2 ** 23 and np.array_equal(X.astype(np.float32).astype(np.float64), X)      # exact in f32
    raw = Raw(dtype, H, G_col)
    ex = seam_mask(m, n_cols, seam)
    pairs = set(map(tuple, ex[:, seam - 1:seam + 1].tolist()))
    assert pairs == {(True, True), (True, False), (False, True), (False, False)} and ex[64:, seam - 1:seam + 1].any()
    assert ex[m - 1, seam] and not ex[5, :seam - 1].any() and ex[5, seam - 1] and not ex[8, seam + 1:].any() and ex[8, seam]
    open_seam = ex.copy()
    open_seam[:, seam - 1:seam + 1] = False                          # what a cursor that loses the seam's entries would see
    what = 'seam %s m %d n %d ranks %r' % (dtype, m, n_cols, ranks)

    hi, hv = host_topk(X, k, ex)
    assert not np.array_equal(hi, host_topk(X, k, open_seam)[0]), 'top-k does not depend on the seam entries'
    got = [raw.topk(k, ex, col_splits=s) for s in (2, 1)]
    for (gi, gv), s in zip(got, (2, 1)):
        assert np.array_equal(gi, hi), '%s top-k splits %d: indices differ from the host order' % (what, s)
        assert np.array_equal(gv.astype(np.float64), hv), '%s top-k splits %d: values differ from the host scores' % (what, s)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*got)), what + ' top-k: two splits and one differ'

    tg = target_mask(m, n_cols)
    tg[::3, seam - 1:seam + 1] = True                                # targets ON the seam, excluded ones among them
    tl = lists_of(tg)
    rows = rows_of(tl)
    assert ex[rows, tl[1]].any() and tg[m - 1, seam - 1:seam + 1].all()
    want = host_ranks(X, tl, ex)
    assert not np.array_equal(want, host_ranks(X, tl, open_seam)), 'the ranks do not depend on the seam entries'
    got = [raw_ranks(raw, tl, ex, col_splits=s) for s in (2, 1)]
    for (gr, gv), s in zip(got, (2, 1)):
        assert np.array_equal(gr, want), '%s ranks splits %d: ranks differ from the host count' % (what, s)
        assert np.array_equal(gv.astype(np.float64), X[rows, tl[1]]), '%s ranks splits %d: values differ from the host scores' % (what, s)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*got)), what + ' ranks: two splits and one differ'

    thr = own_thresholds(X)
    want = host_above(X, thr, ex)
    assert not np.array_equal(want[0], host_above(X, thr, open_seam)[0]), 'above does not depend on the seam entries'
    got = [raw_above(raw, thr, ex, col_splits=s) for s in (2, 1)]
    for g, s in zip(got, (2, 1)):
        same(g, want, '%s above splits %d' % (what, s))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*got)), what + ' above: two splits and one differ'


# ---- 2. agreement with top-k and ranks -------------------------------------------------------------------------------------
def topk_order(idx, val):
    """Positions of a row's entries by (value descending, column ascending); the columns come ascending."""
    return np.argsort(-val, kind='stable')


def check_p2(got, ti, tv, thr, k, what):
    """P2: row r's entries in top-k order start with top-k's list, bit for bit; every further entry equals thr[r]."""
    p, i, v = got
    for r in range(len(p) - 1):
        ri, rv = i[p[r]:p[r + 1]], v[p[r]:p[r + 1]]
        o = topk_order(ri, rv)
        have = int((ti[r] >= 0).sum())
        assert ri.size >= have, '%s row %d: %d entries, top-k holds %d' % (what, r, ri.size, have)
        assert np.array_equal(ri[o[:have]], ti[r, :have]), '%s row %d: the first %d entries are not top-k\'s' % (what, r, have)
        assert rv[o[:have]].tobytes() == tv[r, :have].tobytes(), '%s row %d: value bits differ from top-k\'s' % (what, r)
        assert (rv[o[have:]] == thr[r]).all() and (have == k or ri.size == have), '%s row %d: an entry beyond k is not a tie' % (what, r)


def agreement_case(dtype, m, n_cols, ranks, pattern='edges', factors=lattice_factors):
    G_row, S, G_col = factors(m, n_cols, ranks)
    H = np.dot(G_row, S)
    raw = Raw(dtype, H, G_col)
    ex = exclusion_mask(pattern, m, n_cols)
    what = 'above agreement %s m %d n %d ranks %r %s' % (dtype, m, n_cols, ranks, pattern)
    tl = lists_of(target_mask(m, n_cols))
    trow, tcol = rows_of(tl), tl[1]
    rank, rval = raw_ranks(raw, tl, ex)
    beyond = 0
    for k in (1, 10, 64):
        ti, tv = raw.topk(k, ex, col_splits=2)
        thr = tv[:, k - 1].copy()                                    # (-inf where the row has fewer than k candidates)
        got = raw_above(raw, thr, ex, col_splits=3)
        check_p2(got, ti, tv, thr, k, '%s P2 k %d' % (what, k))
        beyond += int(got[0][-1] - (ti >= 0).sum())
        p, i, v = got
        present = 0
        for e in range(len(tcol)):
            r, j = trow[e], tcol[e]
            ri, rv = i[p[r]:p[r + 1]], v[p[r]:p[r + 1]]
            at = np.nonzero(ri == j)[0]
            if ex is not None and ex[r, j]:
                assert at.size == 0, '%s: the excluded target (%d, %d) is in its row' % (what, r, j)
                continue
            assert (at.size == 1) == bool(rval[e] >= thr[r]), '%s k %d: target (%d, %d) present %d, score %r, thr %r' % (what, k, r, j, at.size, rval[e], thr[r])
            if at.size:
                present += 1
                assert rv[at].tobytes() == rval[e:e + 1].tobytes(), '%s: target (%d, %d): value bits differ from the rank pass' % (what, r, j)
                ahead = int(((rv > rval[e]) | ((rv == rval[e]) & (ri < j))).sum())
                assert ahead == rank[e], '%s k %d: target (%d, %d) has %d entries ahead and rank %d' % (what, k, r, j, ahead, rank[e])
        if k == 64:
            assert present > 0, what + ': no target is present'
    return beyond


# ---- 3. random cases -------------------------------------------------------------------------------------------------------
def midway_thresholds(X64, T):
    """Midway between the (n_cols // 10)-th and the next score of the row, rounded to the scoring type."""
    q = X64.shape[1] // 10
    s = -np.sort(-X64, axis=1)
    return ((s[:, q - 1] + s[:, q]) / 2.0).astype(T)


def check_random(got, X64, B, thr, ex, what, rows=None):
    """The random-case conditions; returns the number of undecided pairs."""
    p, i, v = got
    m, n = X64.shape
    sel = np.zeros((m, n), dtype=bool)
    r_of = np.repeat(np.arange(m), np.diff(p))
    assert (np.diff(p) >= 0).all() and p[0] == 0 and p[-1] == i.size
    for r in range(m):
        assert (np.diff(i[p[r]:p[r + 1]]) > 0).all(), '%s row %d: columns not strictly ascending' % (what, r)
    sel[r_of, i] = True
    ok = np.ones((m, n), dtype=bool) if ex is None else ~ex
    d = X64 - thr.astype(np.float64)[:, None]
    assert not (sel & ~ok).any(), what + ': an excluded pair was selected'
    missing = ok & (d > B) & ~sel
    assert not missing.any(), '%s: %d pairs more than b above the threshold are absent' % (what, missing.sum())
    wrong = sel & (d < -B)
    assert not wrong.any(), '%s: %d pairs more than b below the threshold are present' % (what, wrong.sum())
    ratio = float((np.abs(v - X64[r_of, i]) / B[r_of, i]).max()) if i.size else 0.0
    undecided = int((np.abs(d) <= B).sum())
    print('%s: %d entries, max |value - X64| / b = %.3g, undecided %d of %d pairs' % (what, i.size, ratio, undecided, m * n))
    assert ratio <= 1.0, '%s: a value is %.3e x its bound away' % (what, ratio)
    assert undecided <= 0.001 * m * n, '%s: %d of %d pairs are undecided: the test decides too little' % (what, undecided, m * n)
    return undecided


def random_case(dtype, ranks, m=131, n_cols=997, pattern='edges', label=''):
    G_row, S, G_col = random_factors(m, n_cols, ranks)
    X64 = np.dot(np.dot(G_row, S), G_col.T)
    B = bound(G_row, S, G_col, dtype)
    ex = exclusion_mask(pattern, m, n_cols)
    xl = None if ex is None else lists_of(ex)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    thr = midway_thresholds(X64, comp.npd)
    what = '%s above random %s %dx%d ranks %r %s' % (label, dtype, m, n_cols, ranks, pattern)
    got = comp.above(G_row, thr, exclude=xl)
    check_random(got, X64, B, thr, ex, what)
    for s in (1, 3, 32):
        g2 = comp.above(G_row, thr, exclude=xl, col_splits=s, capacity=7 if s == 3 else None)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, g2)), what + ': col_splits %d changes the bytes' % s
    return got


# ---- 4. NaN -----------------------------------------------------------------------------------------------------------------
def nan_case(dtype, m=67, n_cols=203, ranks=(5, 7)):
    """The input of ranks_cases.nan_case: a NaN in row 9 of H, then one in row 70 of Gc."""
    G_row, S, G_col = lattice_factors(m, n_cols, ranks)
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    rn, jn = 9, 70
    ex = exclusion_mask('edges', m, n_cols)
    thr = own_thresholds(X)
    thr[[rn, 4]] = -np.inf                                           # -inf takes every admissible column whose score is not NaN
    clean = raw_above(Raw(dtype, H, G_col), thr, ex)
    same(clean, host_above(X, thr, ex), 'above NaN: the clean run')
    # a NaN row of H: that row is empty, nobody else notices
    Hn = H.copy()
    Hn[rn, 1] = np.nan
    p, i, v = raw_above(Raw(dtype, Hn, G_col), thr, ex)
    assert p[rn + 1] == p[rn] and clean[0][rn + 1] > clean[0][rn]
    keep = rows_of((clean[0], clean[1])) != rn
    assert np.array_equal(np.diff(p), np.where(np.arange(m) == rn, 0, np.diff(clean[0])))
    assert np.array_equal(i, clean[1][keep]) and v.tobytes() == clean[2][keep].tobytes()
    # a NaN row of Gc: that column is never selected; everything else is as it was
    Gn = G_col.copy()
    Gn[jn, 0] = np.nan
    got = raw_above(Raw(dtype, H, Gn), thr, ex, col_splits=3)
    same(got, host_above(np.dot(H, Gn.T), thr, ex), 'above NaN: a NaN column')
    keep = clean[1] != jn
    assert (~keep).sum() >= 2 and not np.isnan(got[2]).any()
    assert np.array_equal(got[1], clean[1][keep]) and got[2].tobytes() == clean[2][keep].tobytes()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def refusals_without_device(lib, ptr):
    """Everything refused before any HIP call (`ptr`: any non-null, 256-byte aligned address; it is never dereferenced)."""
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    need = C.c_size_t()
    assert lib.skf_complete_above_workspace_bytes(nat.SKF_F32, 67, 203, 0, C.byref(need)) == 0
    nb = need.value
    assert 256 + 67 * 8 <= nb < 16384, 'flag words, the words of the scan and splits x m int64: nothing of the size of the relation'
    found = C.c_int64(-7)

    def above(dtype=nat.SKF_F32, H=ptr, Gc=ptr, c=8, ldh=8, ldg=8, thr=ptr, xp=None, xi=None, cap=100, optr=ptr, oidx=ptr, oval=ptr,
              fnd=C.byref(found), ws=ptr, ws_bytes=nb, splits=0, m=67, n_cols=203):
        return lib.skf_complete_above(dtype, H, ldh, m, Gc, ldg, n_cols, c, thr, xp, xi, cap, optr, oidx, oval, fnd, splits, ws, ws_bytes, None)
    for kw in (dict(dtype=nat.SKF_BF16), dict(dtype=7), dict(m=-1), dict(m=2 ** 31), dict(n_cols=-1), dict(n_cols=2 ** 31), dict(c=0),
               dict(c=1025), dict(H=None), dict(Gc=None), dict(thr=None), dict(optr=None), dict(fnd=None), dict(oidx=None),
               dict(ldh=7), dict(ldg=7), dict(cap=-1), dict(splits=-1), dict(splits=33), dict(xp=ptr), dict(xi=ptr)):
        assert above(**kw) == INV, kw
        assert b'skf_complete_above' in lib.skf_last_error()
        assert found.value == -7, kw
    assert above(ws_bytes=nb - 1) == WS and above(ws=None) == WS and above(ws=ptr + 8) == WS and found.value == -7
    for s in (1, 2, 32):
        assert lib.skf_complete_above_workspace_bytes(nat.SKF_F64, 67, 203, s, C.byref(need)) == 0
        assert need.value >= 256 + min(s, 4) * 67 * 8 and above(dtype=nat.SKF_F64, splits=s, ws_bytes=need.value - 1) == WS, s
    for kw in (dict(splits=33), dict(splits=-1), dict(m=-1), dict(m=2 ** 31), dict(n_cols=2 ** 31), dict(dtype=nat.SKF_BF16)):
        assert lib.skf_complete_above_workspace_bytes(kw.get('dtype', nat.SKF_F32), kw.get('m', 67), kw.get('n_cols', 203),
                                                      kw.get('splits', 0), C.byref(need)) == INV, kw
    assert lib.skf_complete_above_workspace_bytes(nat.SKF_F32, 67, 203, 0, None) == INV
    # 2^31 - 1 rows and 32 splits: the workspace is sized in 64 bits
    assert lib.skf_complete_above_workspace_bytes(nat.SKF_F32, 2 ** 31 - 1, 2 ** 31 - 1, 32, C.byref(need)) == 0
    assert need.value >= 32 * (2 ** 31 - 1) * 8


def refusals_case(dtype='f64'):
    from ranks_cases import defective_lists
    rt = nat.get_runtime()
    keep = rt.mem.empty(16384)
    refusals_without_device(rt.lib, keep.ptr)
    m, n_cols = 37, 70
    G_row, S, G_col = lattice_factors(m, n_cols, (5, 7))
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    raw = Raw(dtype, H, G_col)
    ex = exclusion_mask('edges', m, n_cols)
    xl = lists_of(ex)
    thr = own_thresholds(X)
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    nb = raw_workspace(raw)
    for want, over in ((INV, dict(dtype=nat.SKF_BF16)), (INV, dict(m=-1)), (INV, dict(m=2 ** 31)), (INV, dict(n_cols=-1)),
                       (INV, dict(n_cols=2 ** 31)), (INV, dict(c=0)), (INV, dict(c=1025)), (INV, dict(H=None)), (INV, dict(Gc=None)),
                       (INV, dict(thr=None)), (INV, dict(optr=None)), (INV, dict(found=None)), (INV, dict(oidx=None)),
                       (INV, dict(ldh=raw.c - 1)), (INV, dict(ldg=raw.c - 1)), (INV, dict(cap=-1)), (INV, dict(splits=-1)),
                       (INV, dict(splits=33)), (INV, dict(xp=None)), (INV, dict(xi=None)), (WS, dict(ws_bytes=nb - 1)),
                       (WS, dict(ws=None))):
        res, _ = call_above(raw, thr, xl, **over)
        assert res[0] == want and b'skf_complete_above' in rt.lib.skf_last_error(), over
        assert untouched(res), '%r: an output was written' % (over,)
    # a workspace that is not 256-byte aligned
    mem = rt.mem
    ws = mem.empty(nb + 256)
    res, _ = call_above(raw, thr, xl, ws=ws.ptr + 8, ws_bytes=nb)
    assert res[0] == WS and b'aligned' in rt.lib.skf_last_error() and untouched(res)
    for name, (p, i, n) in defective_lists(xl[0], xl[1], m, n_cols).items():
        if name in ('count does not match indptr[m]', 'indptr does not end at its count'):
            continue                                             # (the exclusion lists carry no count but indptr[m])
        for s in (1, 2):
            res, _ = call_above(raw, thr, (p, i), col_splits=s)
            assert res[0] == INV and b'exclusion lists' in rt.lib.skf_last_error(), 'exclusion: ' + name
            assert untouched(res), 'exclusion: %s: an output was written' % name
    same(raw_above(raw, thr, ex), host_above(X, thr, ex), 'the lists as they were are accepted')


def refusal_order_case(which, dtype='f64'):
    """4 rows x 6 columns with defective exclusion lists: refused by the validation kernel alone."""
    import known_csr_cases as KC
    G_row, S, G_col = lattice_factors(4, 6, (2, 2))
    raw = Raw(dtype, np.dot(G_row, S), G_col)
    KC.refused_after_one_launch(lambda w: raw_above(raw, np.zeros(4), xlists=KC.small_lists(w)), which)


# ---- 6. public API ----------------------------------------------------------------------------------------------------------
def gap_threshold(values, lo, hi):
    """The middle of the widest gap between the sorted `values` from position lo to hi."""
    s = np.sort(np.asarray(values).ravel())[lo:hi]
    g = int(np.argmax(np.diff(s)))
    return (s[g] + s[g + 1]) / 2.0


def csr_of(X, thr, ex=None):
    p, i, v = host_above(X, np.broadcast_to(np.asarray(thr, dtype=np.float64), (X.shape[0],)), ex)
    return p, i, v


def csr_same(got, want, B, what):
    """Pattern exact, values within the bound of the float64 reconstruction."""
    p, i, v = want
    assert got.dtype == np.float64 and got.has_sorted_indices and got.indptr.dtype.kind == 'i', what
    assert np.array_equal(got.indptr, p) and np.array_equal(got.indices, i), what + ': the pattern differs from complete() >= threshold'
    r = np.repeat(np.arange(len(p) - 1), np.diff(p))
    assert (np.abs(got.data - v) <= B[r, i]).all(), what + ': a value is beyond its bound'


def api_case(kind, monkeypatch):
    """kind 'dfmc-masked': Dfmc on a MaskedArray relation; 'dfmf-csr': Dfmf on a scipy.sparse relation (40 x 30, ranks 5 / 4);
    the comparison with complete() runs in f64."""
    import scipy.sparse
    import known_csr_api_cases as KA
    from skfusion_amd.fusion import Dfmc, Dfmf, Relation, ObjectType
    from skfusion_amd.fusion.base import DataFusionError
    csr, ma = KA.ratings(40, 30, 0.2, 11)
    sparse = kind == 'dfmf-csr'
    g, users, movies = KA.graph(csr if sparse else ma, ranks=(5, 4, 3))
    fuser = KA.fit(Dfmf if sparse else Dfmc, g, max_iter=5, init_type='random', random_state=0, dtype='f64')
    rel = list(g.relations)[0]
    known = ~np.ma.getmaskarray(ma)
    pat = scipy.sparse.csr_matrix((np.ones(int(known.sum())), np.nonzero(known)), shape=known.shape)
    fmts = (pat, pat.tocsc(), pat.tocoo())

    def boom(*a, **kw):               # from here on nothing may expand a sparse matrix
        raise AssertionError('a sparse matrix was densified')
    for cls in (scipy.sparse.csr_matrix, scipy.sparse.csc_matrix, scipy.sparse.coo_matrix):
        monkeypatch.setattr(cls, 'toarray', boom)
        monkeypatch.setattr(cls, 'todense', boom)
    X = fuser.complete(rel)
    B = bound(fuser.factor(users), fuser.backbone(rel), fuser.factor(movies), 'f64')
    what = 'api above %s' % kind
    t0 = gap_threshold(X, 800, 1000)                              # a scalar: two thirds of the pairs lie below
    trow = np.array([gap_threshold(X[r], 12, 24) for r in range(40)])
    for thr in (np.full(40, t0), trow):                           # no pair within its bound of a threshold: equality is exact
        assert (np.abs(X - thr[:, None]) > B).all(), what + ': a pair lies within its bound of the threshold'
    full = fuser.complete_above(rel, t0)
    assert scipy.sparse.isspmatrix_csr(full) and full.shape == (40, 30) and 0 < full.nnz < 1200
    csr_same(full, csr_of(X, t0), B, what + ' scalar')
    csr_same(fuser.complete_above(rel, trow), csr_of(X, trow), B, what + ' per row')
    kn = fuser.complete_above(rel, trow, exclude='known')
    csr_same(kn, csr_of(X, trow, known), B, what + " exclude='known'")
    assert kn.nnz < fuser.complete_above(rel, trow).nnz
    for fmt in fmts:
        got = fuser.complete_above(rel, t0, exclude=fmt)
        csr_same(got, csr_of(X, t0, known), B, what + ' exclude= as %s' % fmt.format)
    order = np.array([17, 3, 3, 39, 0])
    got = fuser.complete_above(rel, trow[order], rows=order, exclude='known', block_rows=2)
    assert got.shape == (5, 30)
    csr_same(got, csr_of(X[order], trow[order], known[order]), B, what + ' rows= order')
    sub = kn[order]
    assert np.array_equal(got.indptr, sub.indptr) and np.array_equal(got.indices, sub.indices) and got.data.tobytes() == sub.data.tobytes()
    csr_same(fuser.complete_above(rel, t0, block_rows=7), csr_of(X, t0), B, what + ' block_rows')
    assert fuser.complete_above(rel, np.inf).nnz == 0 and fuser.complete_above(rel, -np.inf, exclude='known').nnz == int((~known).sum())
    assert fuser.complete_above(rel, t0, rows=np.zeros(0, dtype=int)).shape == (0, 30)
    # the result is the next relation / exclusion
    assert fuser.complete_above(rel, -np.inf, exclude=full).nnz == 1200 - full.nnz
    # the size of the result is limited before it is allocated
    assert fuser.complete_above(rel, t0, max_entries=full.nnz).nnz == full.nnz
    for blk in (8192, 7):
        with pytest.raises(DataFusionError, match='max_entries'):
            fuser.complete_above(rel, t0, max_entries=full.nnz - 1, block_rows=blk)
    # 'bf16' scores on the f32 masters
    a, b = fuser.complete_above(rel, trow, exclude='known', dtype='f32'), fuser.complete_above(rel, trow, exclude='known', dtype='bf16')
    assert a.indptr.tobytes() == b.indptr.tobytes() and a.indices.tobytes() == b.indices.tobytes() and a.data.tobytes() == b.data.tobytes()
    assert a.nnz > 0
    # refusals
    with pytest.raises(DataFusionError, match='shape'):
        fuser.complete_above(rel, t0, exclude=pat[:, :20])
    with pytest.raises(DataFusionError):
        fuser.complete_above(rel, t0, rows=[40])
    with pytest.raises(DataFusionError):
        fuser.complete_above(rel, t0, rows=[-1])
    with pytest.raises(DataFusionError):
        fuser.complete_above(rel, t0, rows=[0.5])
    with pytest.raises(DataFusionError):
        fuser.complete_above(rel, trow[:7])
    plain = list(g.relations)[1]                                 # movies x genres: a plain ndarray
    with pytest.raises(DataFusionError, match='plain array'):
        fuser.complete_above(plain, t0, exclude='known')
    stranger = Relation(np.zeros((40, 3)), users, ObjectType('strangers', 2))
    with pytest.raises(DataFusionError):
        fuser.complete_above(stranger, t0)
    post = Relation(rel.data, users, movies, postprocessor=lambda x: np.clip(x, 0.0, 1.0), **({} if not sparse else {'unstored': rel.unstored}))
    fuser.backbones_[post] = fuser.backbones_[rel]
    with pytest.raises(DataFusionError, match='postprocessor'):
        fuser.complete_above(post, t0)
    return fuser


def api_runs_case():
    """n_run = 2 and run=None: a generator over the runs, each equal to the explicit run."""
    import types
    import known_csr_api_cases as KA
    from skfusion_amd.fusion import Dfmc
    _, ma = KA.ratings(40, 30, 0.2, 11)
    g, users, movies = KA.graph(ma, ranks=(5, 4, 3))
    fuser = KA.fit(Dfmc, g, max_iter=3, init_type='random', random_state=0, dtype='f64', n_run=2)
    rel = list(g.relations)[0]
    thr = float(np.median(fuser.complete(rel, run=0)))
    out = fuser.complete_above(rel, thr, exclude='known')
    assert isinstance(out, types.GeneratorType)
    out = list(out)
    assert len(out) == 2
    for r in range(2):
        one = fuser.complete_above(rel, thr, exclude='known', run=r)
        assert np.array_equal(out[r].indptr, one.indptr) and np.array_equal(out[r].indices, one.indices)
        assert out[r].data.tobytes() == one.data.tobytes()
    assert out[0].nnz != out[1].nnz or not np.array_equal(out[0].data, out[1].data)
