"""The k best columns of every row for any k without the dense reconstruction (csrc/skf_complete.h
complete_row_digits_kernel / complete_row_walk_kernel, skf_complete_row_kth, _engine.DeviceCompleter.row_kth / row_best,
FusionFit.complete_row_kth / complete_row_best) -- the SAME cases on the host emulator (small) and on the GPU.  The yardstick is
host NumPy in float64 on factors that are exact in the scoring type: per row a stable sort of the admissible, non-NaN scores by
-score, i.e. by (score descending, column ascending) -- complete_topk's order.

  1. exact cases (lattice factors, a signed variant among them): row_kth's four arrays and complete_row_best's matrix index for
     index and bit for bit, for ties 'first' and 'all', whatever col_splits and block_rows; rows with more pairs at their
     threshold than are wanted of them must occur (the trim).
  2. P5: ordered=True is complete_topk.  3. P4: above at the returned thresholds, every pair of split counts.
  4. random factors: complete_ranks of the selected pairs is 0 .. n_r - 1 per row; values within complete_cases.bound.
  5. NaN and infinities, 6. independence of block_rows / col_splits / the 'bf16' name, 7. exclusion entries on a split seam,
  8. refusals, 10. the public API."""
import ctypes as C

import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DeviceCompleter
from complete_cases import NPT, Raw, bound, exclusion_mask, lattice_factors, lists_of
from best_cases import csr_bytes, model, same_csr, signed_lattice_factors, sparse_of
import best_cases as BC

SPLITS = (0, 1, 2, 3, 32)
BLOCK_ROWS = (64, 8192)
PAD = 3                                          # sentinel elements behind every output
SENT_I = np.int64(0x5A5A5A5A5A5A5A5A)
SENT_F = -7.0


# ---- the host's answer ------------------------------------------------------------------------------------------------------
def wants_of(k, m):
    return np.broadcast_to(np.asarray(k, dtype=np.int64), (m,))


def host_orders(X, ex=None):
    """Per row the candidate columns -- admissible, score not NaN -- in the total order (stable sort by -score)."""
    out = []
    for r in range(X.shape[0]):
        ok = ~np.isnan(X[r])
        if ex is not None:
            ok &= ~ex[r]
        cand = np.nonzero(ok)[0]
        out.append(cand[np.argsort(-X[r, cand], kind='stable')])
    return out


def host_row_kth(X, orders, k):
    """(thr, greater, equal, cands) of the definition, per row."""
    m = X.shape[0]
    want = wants_of(k, m)
    thr = np.full(m, np.nan)
    g, e, cands = (np.zeros(m, dtype=np.int64) for _ in range(3))
    for r, o in enumerate(orders):
        cands[r] = o.size
        n = min(int(want[r]), o.size)
        if n:
            thr[r] = X[r, o[n - 1]]
            g[r] = (X[r, o] > thr[r]).sum()
            e[r] = (X[r, o] == thr[r]).sum()
    return thr, g, e, cands


def host_row_best(X, orders, k, ties='first'):
    """(indptr, indices, values): per row the first min(k_r, cands_r) columns of the order (ties='all': and every further one
    equal to the last of them), columns ascending."""
    m = X.shape[0]
    want = wants_of(k, m)
    thr, g, e, _ = host_row_kth(X, orders, k)
    indptr = np.zeros(m + 1, dtype=np.int64)
    idx, val = [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
    for r, o in enumerate(orders):
        take = int(g[r] + e[r]) if ties == 'all' else min(int(want[r]), o.size)
        cols = np.sort(o[:take])
        indptr[r + 1] = indptr[r] + take
        idx.append(cols)
        val.append(X[r, cols])
    return indptr, np.concatenate(idx).astype(np.int32), np.concatenate(val)


def host_ordered(X, orders, k):
    """complete_topk's layout of the first k of every row's order."""
    idx = np.full((X.shape[0], k), -1, dtype=np.int32)
    val = np.full((X.shape[0], k), -np.inf)
    for r, o in enumerate(orders):
        o = o[:k]
        idx[r, :o.size] = o
        val[r, :o.size] = X[r, o]
    return idx, val


def same_row_kth(got, want, what):
    names = ('thr', 'greater', 'equal', 'cands')
    for name, a, b in zip(names, got, want):
        assert np.asarray(a).dtype == (np.float64 if name == 'thr' else np.int64), '%s: %s has dtype %s' % (what, name, np.asarray(a).dtype)
        assert np.array_equal(a, b, equal_nan=name == 'thr'), '%s: %s differs from the host in rows %r' % (
            what, name, np.nonzero(~((a == b) | ((a != a) & (b != b))))[0][:8])
    real = ~np.isnan(np.asarray(want[0]))
    assert np.asarray(got[0])[real].tobytes() == np.asarray(want[0])[real].tobytes(), what + ': the bits of a threshold differ'


def k_vector(m, cands):
    """One k per row that holds 0, 1, values above the row's candidate count, the count itself and values in between."""
    rs = np.random.RandomState(m)
    k = rs.randint(2, max(3, int(cands.max())), size=m).astype(np.int64)
    k[0::7] = 0
    k[1::7] = 1
    k[2::7] = cands[2::7] + 3
    k[3::7] = cands[3::7]
    return k


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------
def exact_case(dtype, m, n_cols, ranks, signed=False, patterns=('none', 'edges', 'heavy'), ks=None, splits=SPLITS, block_rows=BLOCK_ROWS,
               all_splits_at=(65, 'vector')):
    """Returns the number of (k, row) in which more pairs equal the row's threshold than are wanted of them."""
    G_row, S, G_col = (signed_lattice_factors if signed else lattice_factors)(m, n_cols, ranks)
    X = np.dot(np.dot(G_row, S), G_col.T)
    assert np.abs(X).max() * 512 < 2 ** 23 and np.array_equal(X.astype(np.float32).astype(np.float64), X)      # exact in f32
    assert not signed or ((X < 0).any() and (X[1::2] <= 0).all())
    fit, rel = model(G_row, S, G_col)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    if ks is None:
        ks = (1, 64, 65, 100, n_cols - 1, n_cols, n_cols + 5, 'vector')
    trimmed = 0
    for pattern in patterns:
        ex = exclusion_mask(pattern, m, n_cols)
        xl = None if ex is None else lists_of(ex)
        xs = None if ex is None else sparse_of(ex)
        orders = host_orders(X, ex)
        cands = np.array([o.size for o in orders])
        for k in ks:
            label = k
            k = k_vector(m, cands) if k == 'vector' else k
            what = 'row best exact %s m %d n_cols %d ranks %r signed %d %s k %s' % (dtype, m, n_cols, ranks, signed, pattern, label)
            want = host_row_kth(X, orders, k)
            n_r = np.minimum(wants_of(k, m), cands)
            assert ((want[1] < n_r) & (n_r <= want[1] + want[2]))[n_r > 0].all()
            trimmed += int((want[1] + want[2] > n_r).sum())
            for s in splits if label in all_splits_at else splits[:1]:
                same_row_kth(comp.row_kth(G_row, k, exclude=xl, col_splits=s), want, '%s row_kth splits %d' % (what, s))
            got = fit.complete_row_kth(rel, k, exclude=xs, dtype=dtype, block_rows=64)
            same_row_kth(got + (want[3],), want, what + ' complete_row_kth in blocks of 64')
            for ties in ('first', 'all'):
                hb = host_row_best(X, orders, k, ties)
                assert np.array_equal(np.diff(hb[0]), n_r if ties == 'first' else want[1] + want[2])
                first = None
                for step in block_rows:
                    got = fit.complete_row_best(rel, k, exclude=xs, dtype=dtype, ties=ties, block_rows=step)
                    same_csr(got, hb, '%s ties %s block_rows %d' % (what, ties, step))
                    first = first or csr_bytes(got)
                    assert csr_bytes(got) == first, what + ': block_rows changes the bytes'
    return trimmed


# ---- 2. P5 -------------------------------------------------------------------------------------------------------------------
def p5_case(dtype, m, n_cols, ranks, pattern='edges', factors=lattice_factors, ks=(1, 5, 64), block_rows=BLOCK_ROWS):
    """ordered=True is complete_topk on the same arguments: indices and score bytes, padding included."""
    G_row, S, G_col = factors(m, n_cols, ranks)
    fit, rel = model(G_row, S, G_col)
    ex = exclusion_mask(pattern, m, n_cols)
    xs = None if ex is None else sparse_of(ex)
    padded = 0
    for k in ks:
        ti, tv = fit.complete_topk(rel, k, exclude=xs, dtype=dtype)
        for step in block_rows:
            oi, ov = fit.complete_row_best(rel, k, exclude=xs, dtype=dtype, ordered=True, block_rows=step)
            what = 'P5 %s m %d n_cols %d ranks %r %s k %d block_rows %d' % (dtype, m, n_cols, ranks, pattern, k, step)
            assert oi.dtype == np.int32 and ov.dtype == np.float64 and oi.shape == (m, k) == ov.shape, what
            assert np.array_equal(oi, ti), what + ': not top-k\'s indices'
            assert ov.tobytes() == tv.tobytes(), what + ': not top-k\'s bits'
        padded += int((ti == -1).sum())
    return padded


# ---- 3. P4 -------------------------------------------------------------------------------------------------------------------
def p4_case(dtype, m, n_cols, ranks, pattern='heavy', factors=lattice_factors, ks=(1, 65, 'vector'), splits=SPLITS, cuts=(64, 100)):
    """above(thr) holds greater + equal entries per row, greater of them above thr: for every pair of split counts of the two
    operators and for rows cut into blocks; a NaN threshold selects nothing."""
    G_row, S, G_col = factors(m, n_cols, ranks)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    ex = exclusion_mask(pattern, m, n_cols)
    xl = None if ex is None else lists_of(ex)
    cands = n_cols - (0 if ex is None else ex.sum(axis=1))
    nan_rows = 0
    for k in ks:
        label = k
        k = k_vector(m, cands) if k == 'vector' else k
        for s1 in splits:
            thr, g, e, c = comp.row_kth(G_row, k, exclude=xl, col_splits=s1)
            n_r = np.minimum(wants_of(k, m), c)
            assert np.array_equal(np.isnan(thr), n_r == 0) and ((g < n_r) & (n_r <= g + e))[n_r > 0].all()
            assert (g[n_r == 0] == 0).all() and (e[n_r == 0] == 0).all()
            nan_rows += int(np.isnan(thr).sum())
            what = 'P4 %s m %d n_cols %d ranks %r %s k %s row_kth splits %d' % (dtype, m, n_cols, ranks, pattern, label, s1)
            for s2 in splits:
                p, i, v = comp.above(G_row, thr, exclude=xl, col_splits=s2)
                r_of = np.repeat(np.arange(m), np.diff(p))
                assert np.array_equal(np.diff(p), g + e), '%s above splits %d: entries per row are not greater + equal' % (what, s2)
                assert np.array_equal(np.bincount(r_of[v > thr[r_of]], minlength=m), g), '%s above splits %d: entries above thr' % (what, s2)
        for step in cuts:                                            # the rows cut into blocks, of either operator
            for b0 in range(0, m, step):
                b1 = min(b0 + step, m)
                x = None if xl is None else (xl[0][b0:b1 + 1] - xl[0][b0], xl[1][xl[0][b0]:xl[0][b1]])
                kb = k if np.ndim(k) == 0 else k[b0:b1]
                tb, gb, eb, cb = comp.row_kth(G_row[b0:b1], kb, exclude=x, col_splits=3)
                assert np.array_equal(tb, thr[b0:b1], equal_nan=True) and np.array_equal(gb, g[b0:b1]) and np.array_equal(eb, e[b0:b1])
                assert np.array_equal(np.diff(comp.above(G_row[b0:b1], tb, exclude=x, count_only=True)), gb + eb)
    return nan_rows


# ---- 4. ranks agree ------------------------------------------------------------------------------------------------------------
def ranks_case(dtype, m=67, n_cols=203, ranks=(20, 64), k=100, pattern='heavy'):
    """Random factors: complete_ranks of the pairs complete_row_best selects (ties='first') is, per row, exactly 0 .. n_r - 1
    -- the two operators score with the same product, so no tolerance --, and every value lies within the derived bound
    complete_cases.bound of the float64 host product."""
    T = NPT[dtype]
    G_row, S, G_col = (x.astype(T).astype(np.float64) for x in BC.random_factors(m, n_cols, ranks))      # rounded to the scoring type
    X64 = np.dot(np.dot(G_row, S), G_col.T)
    B = bound(G_row, S, G_col, dtype)
    ex = exclusion_mask(pattern, m, n_cols)
    xs = sparse_of(ex)
    fit, rel = model(G_row, S, G_col)
    got = fit.complete_row_best(rel, k, exclude=xs, dtype=dtype)
    n_r = np.minimum(k, (~ex).sum(axis=1))
    what = 'row best ranks %s %dx%d ranks %r k %d' % (dtype, m, n_cols, ranks, k)
    assert np.array_equal(np.diff(got.indptr), n_r) and (n_r == 0).any() and (n_r == 3).any() and (n_r == k).any(), what
    r_of = np.repeat(np.arange(m), n_r)
    assert not ex[r_of, got.indices].any(), what + ': an excluded pair was selected'
    rank = fit.complete_ranks(rel, r_of, got.indices, exclude=xs, dtype=dtype)
    for r in range(m):
        mine = np.sort(rank[got.indptr[r]:got.indptr[r + 1]])
        assert np.array_equal(mine, np.arange(n_r[r])), '%s row %d: the ranks of the selected pairs are %r' % (what, r, mine[:8])
    ratio = float((np.abs(got.data - X64[r_of, got.indices]) / B[r_of, got.indices]).max())
    print('%s: max |value - X64| / b = %.3g' % (what, ratio))
    assert ratio <= 1.0, '%s: a value is %.3e x its bound away' % (what, ratio)


# ---- 5. NaN and infinities ---------------------------------------------------------------------------------------------------
def nan_inf_case(dtype, m=67, n_cols=203, ranks=(5, 2)):
    """best_cases.nan_inf_case's factors: row 9 scores NaN everywhere, row 4 +inf / NaN, row 11 -inf / NaN; row 20 has every
    column excluded."""
    G_row, S, G_col = lattice_factors(m, n_cols, ranks)
    S[0] = np.maximum(S[0], 0.125)
    G_row[9, 1] = np.nan
    G_row[4] = 0.0
    G_row[4, 0] = np.inf
    G_row[11] = 0.0
    G_row[11, 0] = -np.inf
    with np.errstate(invalid='ignore'):
        X = np.dot(np.dot(G_row, S), G_col.T)
    assert np.isnan(X[9]).all() and np.isposinf(X[4]).sum() > 70 and np.isneginf(X[11]).sum() > 70
    ex = exclusion_mask('edges', m, n_cols)
    ex[20] = True
    xl, xs = lists_of(ex), sparse_of(ex)
    orders = host_orders(X, ex)
    cands = np.array([o.size for o in orders])
    assert cands[9] == 0 and cands[20] == 0 and 0 < cands[4] < n_cols - 40 and 0 < cands[11] < n_cols - 40
    fit, rel = model(G_row, S, G_col)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    for k in (1, 30, int(cands[4]), 100, n_cols + 1):
        what = 'row best NaN / inf %s k %d' % (dtype, k)
        want = host_row_kth(X, orders, k)
        assert np.isnan(want[0][[9, 20]]).all() and want[0][4] == np.inf and want[0][11] == -np.inf
        same_row_kth(comp.row_kth(G_row, k, exclude=xl), want, what)
        for ties in ('first', 'all'):
            for step in (8192, 3):
                got = fit.complete_row_best(rel, k, exclude=xs, dtype=dtype, ties=ties, block_rows=step)
                same_csr(got, host_row_best(X, orders, k, ties), '%s ties %s block_rows %d' % (what, ties, step))
                assert got[9].nnz == 0 and got[20].nnz == 0 and not np.isnan(got.data).any()
                assert got[4].nnz == (min(k, cands[4]) if ties == 'first' else cands[4]) and np.isposinf(got[4].data).all()
                assert np.isneginf(got[11].data).all() and got[11].nnz > 0
    oi, ov = fit.complete_row_best(rel, 30, exclude=xs, dtype=dtype, ordered=True)
    hi, hv = host_ordered(X, orders, 30)
    assert np.array_equal(oi, hi) and ov.tobytes() == hv.tobytes() and (oi[9] == -1).all() and np.isneginf(ov[20]).all()


# ---- 6. independence -----------------------------------------------------------------------------------------------------------
def independence_case(dtype, m=131, n_cols=203, ranks=(20, 64), k=100, pattern='edges', splits=SPLITS, block_rows=BLOCK_ROWS):
    """The bytes of complete_row_best do not depend on block_rows, those of DeviceCompleter.row_best not on col_splits (random
    columns against a coarse row factor: ties survive)."""
    G_row, S, G_col = BC.random_factors(m, n_cols, ranks)
    G_row = np.round(G_row * 16) / 16
    ex = exclusion_mask(pattern, m, n_cols)
    xl, xs = lists_of(ex), sparse_of(ex)
    fit, rel = model(G_row, S, G_col)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    kv = k_vector(m, (~ex).sum(axis=1))
    out = []
    for kk in (k, kv):
        for ties in ('first', 'all'):
            got = [csr_bytes(fit.complete_row_best(rel, kk, exclude=xs, dtype=dtype, ties=ties, block_rows=step)) for step in block_rows]
            assert all(g == got[0] for g in got), 'complete_row_best %s ties %s: block_rows changes the bytes' % (dtype, ties)
            out.append(got[0])
        raw = [comp.row_best(G_row, kk, exclude=xl, col_splits=s) for s in splits]
        for s, res in zip(splits, raw):
            assert all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for a, b in zip(res, raw[0])), \
                'row_best %s: col_splits %d changes the bytes' % (dtype, s)
        assert (raw[0][0].astype(np.int64).tobytes(), raw[0][1].tobytes(), raw[0][2].tobytes()) == out[-1], \
            'row_best %s: not the bytes of complete_row_best(ties=\'all\')' % dtype
        kth = [fit.complete_row_kth(rel, kk, exclude=xs, dtype=dtype, block_rows=step) for step in block_rows]
        assert all(all(np.array_equal(a, b, equal_nan=True) for a, b in zip(t, kth[0])) for t in kth)
    return out


# ---- 7. seam ---------------------------------------------------------------------------------------------------------------------
def seam_case(dtype, m=67, n_cols=203, ranks=(5, 7)):
    """Exclusion entries on the last column of one split and the first of the next (above_cases.seam_mask: columns 127 and 128 of
    two splits of two tiles each), k_r chosen so that row r's k_r-th pair sits in column 127 or 128 wherever the row admits one
    of them: two splits, one split and the host agree, and the host's answer depends on the seam's entries."""
    from above_cases import seam_mask
    seam = 128
    G_row, S, G_col = lattice_factors(m, n_cols, ranks, seed=1)
    X = np.dot(np.dot(G_row, S), G_col.T)
    ex = seam_mask(m, n_cols, seam)
    xl, xs = lists_of(ex), sparse_of(ex)
    orders = host_orders(X, ex)
    k = np.full(m, 70, dtype=np.int64)
    for r, o in enumerate(orders):
        at = np.nonzero((o == seam - 1) | (o == seam))[0]
        if at.size:
            k[r] = at[0] + 1
    assert (k != 70).sum() > m // 2
    open_seam = ex.copy()
    open_seam[:, seam - 1:seam + 1] = False
    loose = host_row_kth(X, host_orders(X, open_seam), k)
    want = host_row_kth(X, orders, k)
    assert not np.array_equal(loose[1], want[1]) or not np.array_equal(loose[2], want[2]), 'the selection does not depend on the seam entries'
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    fit, rel = model(G_row, S, G_col)
    for s in (2, 1):
        same_row_kth(comp.row_kth(G_row, k, exclude=xl, col_splits=s), want, 'row best seam %s splits %d' % (dtype, s))
        p, i, v = comp.row_best(G_row, k, exclude=xl, col_splits=s)[:3]
        hb = host_row_best(X, orders, k, 'all')
        assert np.array_equal(p, hb[0]) and np.array_equal(i, hb[1]) and v.tobytes() == hb[2].tobytes(), 'row best seam %s splits %d' % (dtype, s)
    same_csr(fit.complete_row_best(rel, k, exclude=xs, dtype=dtype), host_row_best(X, orders, k, 'first'), 'row best seam %s' % dtype)


# ---- 8. refusals: the raw entry point -----------------------------------------------------------------------------------------
def row_kth_workspace(raw, col_splits=0):
    need = C.c_size_t()
    raw.rt.call('skf_complete_row_kth_workspace_bytes', raw.code, raw.m, raw.n_cols, col_splits, C.byref(need))
    return need.value


def call_row_kth(raw, wants, xlists=None, col_splits=0, **over):
    """skf_complete_row_kth on the buffers of a complete_cases.Raw: every output starts as sentinels with PAD more behind it, the
    workspace is exactly what the query asks for, filled with 0x5A, with 256 such bytes behind it.  `over` replaces single
    arguments (None: a NULL pointer).  Returns (status, (thr, greater, equal, cands) as they stand [m], everything behind the
    outputs and the workspace intact, the workspace itself untouched)."""
    rt, mem = raw.rt, raw.rt.mem
    m = raw.m
    thr = mem.from_host(np.full(m + PAD, SENT_F, dtype=raw.T))
    outs = [mem.from_host(np.full(m + PAD, SENT_I, dtype=np.int64)) for _ in range(3)]
    need = row_kth_workspace(raw, col_splits if 0 <= col_splits <= 32 else 0)
    ws = mem.from_host(np.full(need + 256, 0x5A, dtype=np.uint8))
    wd = mem.from_host(np.asarray(wants, dtype=np.int64) if len(wants) else np.zeros(1, dtype=np.int64))
    xp = xi = None
    if xlists is not None:
        xp = mem.from_host(np.asarray(xlists[0], dtype=np.int64))
        xi = mem.from_host(np.asarray(xlists[1], dtype=np.int32) if len(xlists[1]) else np.zeros(1, dtype=np.int32))
    a = dict(dtype=raw.code, H=raw.h.ptr, ldh=raw.ldh, m=m, Gc=raw.g.ptr, ldg=raw.ldg, n_cols=raw.n_cols, c=raw.c, want=wd.ptr,
             xp=xp.ptr if xp else None, xi=xi.ptr if xi else None, thr=thr.ptr, greater=outs[0].ptr, equal=outs[1].ptr,
             cands=outs[2].ptr, splits=col_splits, ws=ws.ptr, ws_bytes=need)
    assert set(over) <= set(a), over
    a.update(over)
    rc = rt.lib.skf_complete_row_kth(a['dtype'], a['H'], a['ldh'], a['m'], a['Gc'], a['ldg'], a['n_cols'], a['c'], a['want'], a['xp'],
                                     a['xi'], a['thr'], a['greater'], a['equal'], a['cands'], a['splits'], a['ws'], a['ws_bytes'], mem.stream)
    mem.synchronize()
    t = mem.to_host(thr, (m + PAD,), raw.T)
    o = [mem.to_host(b, (m + PAD,), np.int64) for b in outs]
    w = mem.to_host(ws, (need + 256,), np.uint8)
    intact = bool((t[m:] == SENT_F).all() and all((x[m:] == SENT_I).all() for x in o) and (w[need:] == 0x5A).all())
    return rc, (t[:m].astype(np.float64), o[0][:m].copy(), o[1][:m].copy(), o[2][:m].copy()), intact, bool((w == 0x5A).all())


def untouched(outs, cands=True):
    return bool((outs[0] == SENT_F).all() and (outs[1] == SENT_I).all() and (outs[2] == SENT_I).all() and (not cands or (outs[3] == SENT_I).all()))


def refusals_without_device(lib, ptr):
    """Everything refused before any HIP call (`ptr`: any non-null, 256-byte aligned address; it is never dereferenced)."""
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    need = C.c_size_t()
    assert lib.skf_complete_row_kth_workspace_bytes(nat.SKF_F32, 67, 203, 0, C.byref(need)) == 0
    nb = need.value
    assert 67 * 128 * 4 <= nb <= 67 * (256 * 4 + 16) + 1024, 'flag words, a histogram and two words per row'
    big = C.c_size_t()
    assert lib.skf_complete_row_kth_workspace_bytes(nat.SKF_F32, 67, 2 ** 31 - 1, 32, C.byref(big)) == 0 and big.value == nb, \
        'the workspace grows with m, never with n_cols or the splits'
    assert lib.skf_complete_row_kth_workspace_bytes(nat.SKF_F64, 670, 203, 0, C.byref(big)) == 0 and big.value < 10 * nb

    def kth(dtype=nat.SKF_F32, H=ptr, Gc=ptr, c=8, ldh=8, ldg=8, want=ptr, xp=None, xi=None, thr=ptr, greater=ptr, equal=ptr, cands=ptr,
            ws=ptr, ws_bytes=nb, splits=0, m=67, n_cols=203):
        return lib.skf_complete_row_kth(dtype, H, ldh, m, Gc, ldg, n_cols, c, want, xp, xi, thr, greater, equal, cands, splits, ws, ws_bytes, None)
    for kw in (dict(dtype=nat.SKF_BF16), dict(dtype=7), dict(m=-1), dict(m=2 ** 31), dict(n_cols=-1), dict(n_cols=2 ** 31), dict(c=0),
               dict(c=1025), dict(H=None), dict(Gc=None), dict(want=None), dict(thr=None), dict(greater=None), dict(equal=None),
               dict(ldh=7), dict(ldg=7), dict(splits=-1), dict(splits=33), dict(xp=ptr), dict(xi=ptr)):
        assert kth(**kw) == INV, kw
        assert b'skf_complete_row_kth' in lib.skf_last_error(), kw
    assert kth(ws_bytes=nb - 1) == WS and kth(ws=None) == WS and kth(ws=ptr + 8) == WS
    assert b'skf_complete_row_kth' in lib.skf_last_error()
    for kw in (dict(splits=33), dict(splits=-1), dict(m=-1), dict(m=2 ** 31), dict(n_cols=2 ** 31), dict(dtype=nat.SKF_BF16)):
        assert lib.skf_complete_row_kth_workspace_bytes(kw.get('dtype', nat.SKF_F32), kw.get('m', 67), kw.get('n_cols', 203),
                                                        kw.get('splits', 0), C.byref(need)) == INV, kw
    assert lib.skf_complete_row_kth_workspace_bytes(nat.SKF_F32, 67, 203, 0, None) == INV


def refusals_case(dtype='f64', m=67, n_cols=70):
    """Every refusal of the entry point leaves every output and the workspace as they were, the invalid exclusion lists and a
    negative want included: those are refused after the validation launches alone, before anything is counted."""
    from ranks_cases import defective_lists
    from skfusion_amd._engine import launch_count
    rt = nat.get_runtime()
    keep = rt.mem.empty(16384)
    refusals_without_device(rt.lib, keep.ptr)
    G_row, S, G_col = lattice_factors(m, n_cols, (5, 7))
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    raw = Raw(dtype, H, G_col)
    ex = exclusion_mask('edges', m, n_cols)
    xl = lists_of(ex)
    want = np.full(m, 9, dtype=np.int64)
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    nb = row_kth_workspace(raw)
    for status, over in ((INV, dict(dtype=nat.SKF_BF16)), (INV, dict(m=-1)), (INV, dict(m=2 ** 31)), (INV, dict(n_cols=-1)),
                         (INV, dict(n_cols=2 ** 31)), (INV, dict(c=0)), (INV, dict(c=1025)), (INV, dict(H=None)), (INV, dict(Gc=None)),
                         (INV, dict(want=None)), (INV, dict(thr=None)), (INV, dict(greater=None)), (INV, dict(equal=None)),
                         (INV, dict(ldh=raw.c - 1)), (INV, dict(ldg=raw.c - 1)), (INV, dict(splits=-1)), (INV, dict(splits=33)),
                         (INV, dict(xp=None)), (INV, dict(xi=None)), (WS, dict(ws_bytes=nb - 1)), (WS, dict(ws=None))):
        before = launch_count()
        rc, outs, intact, ws_same = call_row_kth(raw, want, xl, **over)
        assert rc == status and b'skf_complete_row_kth' in rt.lib.skf_last_error(), over
        assert launch_count() == before, '%r: refused after a launch' % (over,)
        assert untouched(outs) and intact and ws_same, '%r: an output or the workspace was written' % (over,)
    ws = rt.mem.from_host(np.full(nb + 512, 0x5A, dtype=np.uint8))
    rc, outs, intact, _ = call_row_kth(raw, want, xl, ws=ws.ptr + 8, ws_bytes=nb)
    assert rc == WS and b'aligned' in rt.lib.skf_last_error() and untouched(outs) and intact
    assert (rt.mem.to_host(ws, (nb + 512,), np.uint8) == 0x5A).all()
    # found on the device, before anything is counted: only the flag word of the workspace is written
    for name, (p, i, n) in defective_lists(xl[0], xl[1], m, n_cols).items():
        if name in ('count does not match indptr[m]', 'indptr does not end at its count'):
            continue                                             # (the exclusion lists carry no count but indptr[m])
        for s in (1, 2):
            before = launch_count()
            rc, outs, intact, _ = call_row_kth(raw, want, (p, i), col_splits=s)
            assert rc == INV and b'exclusion lists' in rt.lib.skf_last_error(), 'exclusion: ' + name
            assert launch_count() - before <= 2, 'exclusion: %s: something ran after the validation' % name
            assert untouched(outs) and intact, 'exclusion: %s: an output was written' % name
    for where in (0, m // 2, m - 1):
        neg = want.copy()
        neg[where] = -1
        for lists in (xl, None):
            before = launch_count()
            rc, outs, intact, _ = call_row_kth(raw, neg, lists)
            assert rc == INV and b'negative' in rt.lib.skf_last_error(), 'want[%d] = -1' % where
            assert launch_count() - before == (2 if lists else 1), 'want[%d] = -1: something ran after the validation' % where
            assert untouched(outs) and intact, 'want[%d] = -1: an output was written' % where
    # the same buffers, accepted: the host's answer, nothing behind the outputs; without out_cands too
    orders = host_orders(X, ex)
    hw = host_row_kth(X, orders, want)
    for over in ({}, dict(cands=None)):
        rc, outs, intact, _ = call_row_kth(raw, want, xl, **over)
        rt.check(rc)
        assert intact, 'memory behind an output or behind the workspace changed'
        same_row_kth(outs[:3], hw[:3], 'raw row_kth %s' % dtype)
        assert np.array_equal(outs[3], hw[3]) if not over else (outs[3] == SENT_I).all()
    # no row: success, nothing written; no column: success without a product launch, every row NaN / 0
    rc, outs, intact, ws_same = call_row_kth(Raw(dtype, H[:0], G_col), want[:0])
    assert rc == 0 and intact and ws_same
    before = launch_count()
    rc, outs, intact, _ = call_row_kth(Raw(dtype, H, G_col[:0]), want)
    assert rc == 0 and intact and launch_count() - before <= 2
    assert np.isnan(outs[0]).all() and not outs[1].any() and not outs[2].any() and not outs[3].any()


def refusal_order_case(which, dtype='f64'):
    """4 rows x 6 columns with defective exclusion lists: SKF_E_INVALID after the two validation launches (the lists, the wants)
    and nothing else; the canonical lists are accepted afterwards."""
    import known_csr_cases as KC
    from skfusion_amd._engine import launch_count
    G_row, S, G_col = lattice_factors(4, 6, (2, 2))
    raw = Raw(dtype, np.dot(G_row, S), G_col)
    before = launch_count()
    rc, outs, intact, _ = call_row_kth(raw, [2, 2, 2, 2], KC.small_lists(which))
    assert rc == nat.SKF_E_INVALID and launch_count() - before == 2 and untouched(outs) and intact
    rc, outs, intact, _ = call_row_kth(raw, [2, 2, 2, 2], KC.small_lists('ok'))
    assert rc == 0 and intact and np.array_equal(outs[3], [4, 4, 6, 4])


def engine_refusals_case(dtype='f32'):
    """What DeviceCompleter.row_kth / row_best refuse on the host."""
    G_row, S, G_col = lattice_factors(9, 20, (5, 7))
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    for method in (comp.row_kth, comp.row_best):
        for k in (-1, 2.5, [1] * 8, np.ones((9, 1), dtype=int), [1] * 8 + [-1]):
            with pytest.raises(ValueError):
                method(G_row, k)
        with pytest.raises(ValueError):
            method(G_row, 3, exclude=(np.zeros(9, dtype=np.int64), np.zeros(0, dtype=np.int32)))
        with pytest.raises(ValueError):
            method(G_row[:, :4], 3)
    from skfusion_amd._engine import AboveLimit
    with pytest.raises(AboveLimit) as over:
        comp.row_best(G_row, 5, max_entries=44)
    assert over.value.found >= 45
    assert comp.row_best(G_row, 5, max_entries=9 * 20)[0][-1] >= 45
    empty = comp.row_best(G_row[:0], 5)
    assert empty[0].tolist() == [0] and all(x.size == 0 for x in empty[1:]) and all(x.size == 0 for x in comp.row_kth(G_row[:0], 5))


# ---- 10. public API ----------------------------------------------------------------------------------------------------------
def api_case(kind, monkeypatch):
    """The fitted models of above_cases.api_case ('dfmc-masked' with exclude='known', 'dfmf-csr') with factors rounded to a
    coarse lattice, so that the host order is exact in f64: complete_row_kth, complete_row_best and complete_above agree with the
    host and with each other; rows= in a shuffled order with a duplicate; every DataFusionError."""
    import scipy.sparse
    import above_cases as AC
    from skfusion_amd.fusion import Relation
    from skfusion_amd.fusion.base import DataFusionError, FusionFit
    fuser = AC.api_case(kind, monkeypatch)                           # (sparse matrices can no longer be expanded)
    rel = list(fuser.fusion_graph.relations)[0]
    users, movies = rel.row_type, rel.col_type
    for t in (users, movies):                                        # multiples of 1/64: every partial sum is exact
        fuser.factors_[t] = [np.round(np.asarray(G) * 64) / 64 for G in fuser.factors_[t]]
    fuser.backbones_[rel] = [np.round(np.asarray(S) * 64) / 64 for S in fuser.backbones_[rel]]
    X = np.dot(np.dot(fuser.factor(users), fuser.backbone(rel)), fuser.factor(movies).T)
    n_i, n_j = X.shape
    data = rel.data
    known = ~np.ma.getmaskarray(data) if np.ma.isMaskedArray(data) else BC._pattern(data)
    what = 'api row best %s' % kind

    def boom(*a, **kw):
        raise AssertionError('the dense reconstruction was formed')
    monkeypatch.setattr(FusionFit, 'complete', boom)
    monkeypatch.setattr(FusionFit, '_reconstruct', boom)
    kv = k_vector(n_i, np.full(n_i, n_j))
    for exclude, ex in ((None, None), ('known', known)):
        orders = host_orders(X, ex)
        for k in (1, 7, n_j + 2, kv):
            want = host_row_kth(X, orders, k)
            got = fuser.complete_row_kth(rel, k, exclude=exclude, block_rows=7)
            same_row_kth(got + (want[3],), want, '%s kth' % what)
            above = fuser.complete_above(rel, got[0], exclude=exclude)
            assert np.array_equal(np.diff(above.indptr), got[1] + got[2]), what + ': complete_above at the thresholds'
            for ties in ('first', 'all'):
                best = fuser.complete_row_best(rel, k, exclude=exclude, ties=ties, block_rows=7)
                same_csr(best, host_row_best(X, orders, k, ties), '%s ties %s' % (what, ties))
            assert csr_bytes(best) == csr_bytes(above), what + ': ties=\'all\' is complete_above at complete_row_kth\'s thresholds'
    # rows in a shuffled order with a duplicate: a row listed twice is two rows
    rows = np.array([17, 3, 3, 39, 0])
    orders = host_orders(X[rows], known[rows])
    for k in (1, 10, np.array([0, 4, 9, 50, 2])):
        got = fuser.complete_row_best(rel, k, rows=rows, exclude='known', block_rows=2)
        same_csr(got, host_row_best(X[rows], orders, k), '%s rows=' % what)
        assert csr_bytes(got[1]) == csr_bytes(got[2]) or np.ndim(k)
        kth = fuser.complete_row_kth(rel, k, rows=rows, exclude='known', block_rows=2)
        same_row_kth(kth, host_row_kth(X[rows], orders, k)[:3], '%s rows= kth' % what)
        above = fuser.complete_above(rel, kth[0], rows=rows, exclude='known')
        assert np.array_equal(np.diff(above.indptr), kth[1] + kth[2])
    oi, ov = fuser.complete_row_best(rel, 6, rows=rows, exclude='known', ordered=True, block_rows=2)
    ti, tv = fuser.complete_topk(rel, 6, rows=rows, exclude='known', block_rows=2)
    assert np.array_equal(oi, ti) and ov.tobytes() == tv.tobytes(), what + ': ordered=True is not complete_topk'
    # k = 0, no rows, more than a row holds, the result as the next exclusion
    assert fuser.complete_row_best(rel, 0).nnz == 0 and fuser.complete_row_best(rel, 0).shape == (n_i, n_j)
    T, g, e = fuser.complete_row_kth(rel, 0)
    assert np.isnan(T).all() and not g.any() and not e.any()
    assert fuser.complete_row_best(rel, 5, rows=np.zeros(0, dtype=int)).shape == (0, n_j)
    assert all(x.shape == (0,) for x in fuser.complete_row_kth(rel, 5, rows=np.zeros(0, dtype=int)))
    oi, ov = fuser.complete_row_best(rel, 3, rows=np.zeros(0, dtype=int), ordered=True)
    assert oi.shape == (0, 3) and ov.shape == (0, 3)
    assert fuser.complete_row_best(rel, 2 * n_j).nnz == n_i * n_j
    top = fuser.complete_row_best(rel, 4)
    nxt = fuser.complete_row_best(rel, 4, exclude=top)
    assert nxt.nnz == 4 * n_i and top.multiply(nxt).nnz == 0
    rmin = np.minimum.reduceat(top.data, top.indptr[:-1])
    rmax = np.maximum.reduceat(nxt.data, nxt.indptr[:-1])
    assert (rmax <= rmin).all(), what + ': the next four of a row beat its first four'
    # 'bf16' scores on the f32 masters
    a = fuser.complete_row_best(rel, 9, exclude='known', dtype='f32')
    b = fuser.complete_row_best(rel, 9, exclude='known', dtype='bf16')
    assert csr_bytes(a) == csr_bytes(b) and a.nnz > 0
    # refusals
    for method in (fuser.complete_row_best, fuser.complete_row_kth):
        with pytest.raises(DataFusionError, match='negative'):
            method(rel, -1)
        with pytest.raises(DataFusionError, match='negative'):
            method(rel, np.where(np.arange(n_i) == 5, -2, 3))
        with pytest.raises(DataFusionError, match='integer'):
            method(rel, 2.5)
        with pytest.raises(DataFusionError, match='integer'):
            method(rel, np.full(n_i, 2.0))
        with pytest.raises(DataFusionError, match='shape'):
            method(rel, np.full(n_i - 1, 2))
        with pytest.raises(DataFusionError, match='shape'):
            method(rel, np.full((n_i, 1), 2))
        with pytest.raises(DataFusionError, match='shape'):
            method(rel, np.full(n_i, 2), rows=rows)
        with pytest.raises(DataFusionError):
            method(rel, 10, rows=[n_i])
        with pytest.raises(DataFusionError, match='shape'):
            method(rel, 10, exclude=scipy.sparse.csr_matrix((n_i, n_j - 1)))
    with pytest.raises(DataFusionError, match='ties'):
        fuser.complete_row_best(rel, 10, ties='last')
    with pytest.raises(DataFusionError, match='ordered'):
        fuser.complete_row_best(rel, 10, ordered='yes')
    with pytest.raises(DataFusionError, match='ordered'):
        fuser.complete_row_best(rel, 10, ordered=True, ties='all')
    with pytest.raises(DataFusionError, match='ordered'):
        fuser.complete_row_best(rel, np.full(n_i, 3), ordered=True)
    with pytest.raises(DataFusionError, match='max_entries'):
        fuser.complete_row_best(rel, 2, max_entries=2 * n_i - 1)
    assert fuser.complete_row_best(rel, n_j + 9, max_entries=n_i * n_j).nnz == n_i * n_j       # (min(k, n_j) counts)
    # a block whose ties push the result beyond max_entries: rows 3 and 3 again hold the same scores; a lattice of 1/2 ties
    fuser.backbones_[rel] = [np.round(np.asarray(S) * 2) / 2 for S in fuser.backbones_[rel]]
    for t in (users, movies):
        fuser.factors_[t] = [np.round(np.asarray(G) * 2) / 2 for G in fuser.factors_[t]]
    thr, g, e = fuser.complete_row_kth(rel, 1)
    assert (g + e).sum() > n_i, what + ': no ties on the coarse lattice'
    with pytest.raises(DataFusionError, match='max_entries'):
        fuser.complete_row_best(rel, 1, max_entries=n_i)
    with pytest.raises(DataFusionError, match='max_entries'):
        fuser.complete_row_best(rel, 1, max_entries=n_i, ties='all')
    assert fuser.complete_row_best(rel, 1, max_entries=int((g + e).sum())).nnz == n_i
    post = Relation(rel.data, users, movies, postprocessor=lambda x: np.clip(x, 0.0, 1.0),
                    **({'unstored': rel.unstored} if scipy.sparse.issparse(rel.data) else {}))
    fuser.backbones_[post] = fuser.backbones_[rel]
    for method in (fuser.complete_row_best, fuser.complete_row_kth):
        with pytest.raises(DataFusionError, match='postprocessor'):
            method(post, 10)


def api_runs_case():
    """n_run = 2 and run=None: a generator over the runs, each equal to the explicit run."""
    import types
    import known_csr_api_cases as KA
    from skfusion_amd.fusion import Dfmc
    _, ma = KA.ratings(40, 30, 0.2, 11)
    g, users, movies = KA.graph(ma, ranks=(5, 4, 3))
    fuser = KA.fit(Dfmc, g, max_iter=3, init_type='random', random_state=0, dtype='f64', n_run=2)
    rel = list(g.relations)[0]
    out, kth = fuser.complete_row_best(rel, 8, exclude='known'), fuser.complete_row_kth(rel, 8, exclude='known')
    assert isinstance(out, types.GeneratorType) and isinstance(kth, types.GeneratorType)
    out, kth = list(out), list(kth)
    assert len(out) == len(kth) == 2
    for r in range(2):
        one = fuser.complete_row_best(rel, 8, exclude='known', run=r)
        assert csr_bytes(out[r]) == csr_bytes(one) and (np.diff(one.indptr) <= 8).all() and one.nnz > 0
        k1 = fuser.complete_row_kth(rel, 8, exclude='known', run=r)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(kth[r], k1))
        has = np.diff(one.indptr) > 0
        assert np.array_equal(np.minimum.reduceat(one.data, one.indptr[:-1][has]), k1[0][has])
    assert csr_bytes(out[0]) != csr_bytes(out[1])
    oi = fuser.complete_row_best(rel, 8, exclude='known', ordered=True)
    assert isinstance(oi, types.GeneratorType) and len(list(oi)) == 2
