"""Score histograms and ROC / PR curves without the dense reconstruction (csrc/skf_complete.h complete_hist_kernel,
skf_complete_hist, _engine.DeviceCompleter.hist / histogram, FusionFit.complete_histogram / complete_curve) -- the SAME cases on
the host emulator (small) and on the GPU.  The yardstick is host NumPy in float64 on factors rounded to the scoring type:
    bin(s) = #{ t : edges[t] <= s } = np.searchsorted(edges, s, side='right')
over the candidates -- admissible, not NaN.

  1. exact cases (lattice factors, a signed variant among them: every partial sum exact): both histograms equal np.bincount of
     the host's bins, added to a non-zero prefill, sentinels behind both, whatever col_splits; more than 2047 edges in walks.
  2. P6 against skf_complete_above (count only), P7 against skf_complete_ranks' out_val.
  3. random cases under the derived bound B = max complete_cases.bound: for every edge e the count at or above it lies between
     #{X64 >= e + B} and #{X64 >= e - B}; the same for the targets.
  4. NaN and infinities, 5. independence of block_rows / col_splits / the 'bf16' name, 6. refusals, 7. the public API."""
import ctypes as C
import fractions

import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DeviceCompleter, launch_count
from complete_cases import NPT, Raw, bound, exclusion_mask, lattice_factors, lists_of, random_factors
from ranks_cases import defective_lists, raw_ranks, rows_of, target_mask
from above_cases import raw_above
from best_cases import PAD, SENT, SPLITS, blocks_of, model, signed_lattice_factors, sparse_of

MAX_EDGES = 2047
DEVIATIONS = []                                  # lines of the random cases (the GPU module prints them at the end)


# ---- the host's answer ------------------------------------------------------------------------------------------------------
def in_type(edges, dtype):
    """`edges` as the device compares them: cast to the scoring type, as float64."""
    return np.asarray(edges, dtype=np.float64).astype(NPT[dtype]).astype(np.float64)


def host_hist(X, edges, ex=None, tg=None):
    """(counts, target counts or None) int64 [len(edges) + 1] of the definition on the float64 scores X."""
    ok = ~np.isnan(X)
    if ex is not None:
        ok &= ~ex
    n = len(edges) + 1
    h = np.bincount(np.searchsorted(edges, X[ok], side='right'), minlength=n).astype(np.int64)
    if tg is None:
        return h, None
    return h, np.bincount(np.searchsorted(edges, X[ok & tg], side='right'), minlength=n).astype(np.int64)


def at_or_above(counts):
    """counts at or above every edge: the sum of the bins above t, in Python integers."""
    run, out = 0, []
    for v in reversed([int(c) for c in counts[1:]]):
        run += v
        out.append(run)
    return out[::-1]


def edge_sets(X, dtype, signed=False):
    """name -> edges (float64, already in the scoring type): what the issue lists."""
    u = np.unique(X[~np.isnan(X)])
    pick = u if u.size <= MAX_EDGES else u[np.unique(np.linspace(0, u.size - 1, MAX_EDGES).astype(np.int64))]
    sets = {'every distinct score': pick,
            'one edge': u[u.size // 2:u.size // 2 + 1],
            'exactly 2047 edges': in_type(np.linspace(u[0] - 1.0, u[-1] + 1.0, MAX_EDGES), dtype),
            'duplicates': np.repeat(pick[::max(1, pick.size // 300)], 2),
            '-inf first and +inf last': np.concatenate([[-np.inf], pick[::max(1, pick.size // 50)], [np.inf]])}
    if u.size > 1:
        mid = in_type((u[:-1] + u[1:]) / 2.0, dtype)
        sets['midway between scores'] = mid[np.unique(np.linspace(0, mid.size - 1, min(mid.size, MAX_EDGES)).astype(np.int64))]
    if signed:
        assert (X < 0).any() and (X == 0).any(), 'no zero score on the signed lattice'
        below = u[u < 0].max()
        sets['-0.0 then +0.0'] = np.array([below, -0.0, 0.0, 1.0 / 512])
        sets['+0.0 then -0.0'] = np.array([below, 0.0, -0.0, 1.0 / 512])
    for name, e in sets.items():
        assert 1 <= e.size <= MAX_EDGES and np.array_equal(in_type(e, dtype), e) and not (e[1:] < e[:-1]).any(), name
    assert sets['exactly 2047 edges'].size == MAX_EDGES
    return sets


# ---- the C ABI, called directly ----------------------------------------------------------------------------------------------
def hist_workspace(raw, n_targets=0, col_splits=0):
    need = C.c_size_t()
    raw.rt.call('skf_complete_hist_workspace_bytes', raw.code, raw.m, raw.n_cols, n_targets, col_splits, C.byref(need))
    return need.value


def _lists_on_device(mem, lists):
    if lists is None:
        return None, None
    return (mem.from_host(np.asarray(lists[0], dtype=np.int64)),
            mem.from_host(np.asarray(lists[1], dtype=np.int32) if len(lists[1]) else np.zeros(1, dtype=np.int32)))


def call_hist(raw, edges, xlists=None, tlists=None, col_splits=0, start=None, start_tgt=None, n_targets=None, **over):
    """skf_complete_hist on the buffers of a complete_cases.Raw: the histograms start as `start` / `start_tgt` (default: zeros)
    with PAD sentinel words behind each (the target histogram is there, and must stay, also without targets), the workspace is
    exactly what the query asks for with 256 sentinel bytes behind it.  `over` replaces single arguments (None: a NULL
    pointer).  Returns (status, hist [n + 1], hist_tgt [n + 1], every sentinel intact, the workspace itself untouched)."""
    rt, mem = raw.rt, raw.rt.mem
    e = np.asarray(edges, dtype=raw.T)
    n = e.size
    h0 = np.zeros(n + 1, dtype=np.uint64) if start is None else np.asarray(start, dtype=np.uint64)
    t0 = np.zeros(n + 1, dtype=np.uint64) if start_tgt is None else np.asarray(start_tgt, dtype=np.uint64)
    pad = np.full(PAD, SENT, dtype=np.uint64)
    be = mem.from_host(e if n else np.zeros(1, dtype=raw.T))
    hist, hist_tgt = mem.from_host(np.concatenate([h0, pad])), mem.from_host(np.concatenate([t0, pad]))
    nt = (len(tlists[1]) if tlists is not None else 0) if n_targets is None else n_targets
    need = hist_workspace(raw, max(nt, 0), col_splits if 0 <= col_splits <= 32 else 0)
    ws = mem.from_host(np.full(need + 256, 0x5A, dtype=np.uint8))
    xp, xi = _lists_on_device(mem, xlists)
    tp, ti = _lists_on_device(mem, tlists)
    a = dict(dtype=raw.code, H=raw.h.ptr, ldh=raw.ldh, m=raw.m, Gc=raw.g.ptr, ldg=raw.ldg, n_cols=raw.n_cols, c=raw.c, edge_ptr=be.ptr,
             n_edges=n, xp=xp.ptr if xp else None, xi=xi.ptr if xi else None, tp=tp.ptr if tp else None, ti=ti.ptr if ti else None,
             n_targets=nt, hist=hist.ptr, hist_tgt=hist_tgt.ptr if tp else None, splits=col_splits, ws=ws.ptr, ws_bytes=need)
    assert set(over) <= set(a), over
    a.update(over)
    rc = rt.lib.skf_complete_hist(a['dtype'], a['H'], a['ldh'], a['m'], a['Gc'], a['ldg'], a['n_cols'], a['c'], a['edge_ptr'], a['n_edges'],
                                  a['xp'], a['xi'], a['tp'], a['ti'], a['n_targets'], a['hist'], a['hist_tgt'], a['splits'], a['ws'],
                                  a['ws_bytes'], mem.stream)
    mem.synchronize()
    h, t = mem.to_host(hist, (n + 1 + PAD,), np.uint64), mem.to_host(hist_tgt, (n + 1 + PAD,), np.uint64)
    w = mem.to_host(ws, (need + 256,), np.uint8)
    intact = bool((h[n + 1:] == SENT).all() and (t[n + 1:] == SENT).all() and (w[need:] == 0x5A).all())
    return rc, h[:n + 1].copy(), t[:n + 1].copy(), intact, bool((w[:need] == 0x5A).all())


def raw_hist(raw, edges, ex=None, tg=None, col_splits=0, start=None, start_tgt=None, xlists=None, tlists=None):
    """A successful call: the increments (hist, hist_tgt or None) as int64."""
    if xlists is None and ex is not None:
        xlists = lists_of(ex)
    if tlists is None and tg is not None:
        tlists = lists_of(tg)
    n = len(edges)
    s0 = np.zeros(n + 1, dtype=np.uint64) if start is None else np.asarray(start, dtype=np.uint64)
    s1 = np.zeros(n + 1, dtype=np.uint64) if start_tgt is None else np.asarray(start_tgt, dtype=np.uint64)
    rc, h, t, intact, _ = call_hist(raw, edges, xlists, tlists, col_splits, s0, s1)
    raw.rt.check(rc)
    assert intact, 'memory behind a histogram or behind the workspace changed'
    assert (h >= s0).all() and (t >= s1).all(), 'a histogram was cleared, not added to'
    if tlists is None:
        assert np.array_equal(t, s1), 'no targets and the buffer beside the histogram changed'
        return (h - s0).astype(np.int64), None
    return (h - s0).astype(np.int64), (t - s1).astype(np.int64)


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------
def factors_of(m, n_cols, ranks, signed=False, seed=0):
    """The lattice factors; signed: best_cases' variant with rows 2 and 5 of the row factor cleared -- zero scores, from an even
    row (+0.0) and from a negated one (the products are -0.0, the accumulators start at +0.0)."""
    if not signed:
        return lattice_factors(m, n_cols, ranks, seed)
    G_row, S, G_col = signed_lattice_factors(m, n_cols, ranks, seed)
    G_row[2] *= 0.0
    G_row[5] *= 0.0
    assert np.signbit(G_row[5]).any() and not np.signbit(G_row[2]).any()
    return G_row, S, G_col


def exact_case(dtype, m, n_cols, ranks, signed=False, patterns=('none', 'edges', 'heavy'), splits=SPLITS):
    """Raw ABI: both histograms against the host, added to a non-zero prefill, for every edge set; every col_splits on the
    edge set of every distinct score, two of them on the others."""
    G_row, S, G_col = factors_of(m, n_cols, ranks, signed)
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    assert np.abs(X).max() * 512 < 2 ** 23 and np.array_equal(X.astype(np.float32).astype(np.float64), X)      # exact in f32
    raw = Raw(dtype, H, G_col)
    tg = target_mask(m, n_cols)
    sets = edge_sets(X, dtype, signed)
    if ranks == (5, 1) and (m, n_cols) == (131, 997) and not signed:
        assert sets['every distinct score'].size == 220
    for pattern in patterns:
        ex = exclusion_mask(pattern, m, n_cols)
        if ex is not None:
            assert (ex & tg).any(), 'no target is itself excluded'
        for name, e in sets.items():
            what = 'hist exact %s m %d n_cols %d ranks %r signed %d %s, %s' % (dtype, m, n_cols, ranks, signed, pattern, name)
            want, want_t = host_hist(X, e, ex, tg)
            assert want.sum() == (m * n_cols if ex is None else (~ex).sum()) and 0 < want_t.sum() <= tg.sum()
            start = np.arange(e.size + 1, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
            start_t = np.arange(e.size + 1, dtype=np.uint64) * np.uint64(5) + np.uint64(2)
            for s in splits if name == 'every distinct score' else (splits[0], splits[-2]):
                got, got_t = raw_hist(raw, e, ex, tg, col_splits=s, start=start, start_tgt=start_t)
                assert np.array_equal(got, want), '%s splits %d: the histogram differs from the host' % (what, s)
                assert np.array_equal(got_t, want_t), '%s splits %d: the target histogram differs from the host' % (what, s)
            got, none = raw_hist(raw, e, ex, None, start=start)
            assert none is None and np.array_equal(got, want), what + ': without targets'
    # no row, no column: success, nothing added
    e = sets['one edge']
    start = np.array([7, 9], dtype=np.uint64)
    for empty in (Raw(dtype, H[:0], G_col), Raw(dtype, H, G_col[:0])):
        got, got_t = raw_hist(empty, e, None, np.zeros((empty.m, empty.n_cols), dtype=bool), start=start, start_tgt=start)
        assert not got.any() and not got_t.any()


def walks_case(dtype, m, n_cols, ranks=(5, 7), pattern='edges', n_distinct=None):
    """More than 2047 edges -- every distinct score -- through DeviceCompleter.histogram and complete_histogram: one walk per
    chunk, merged on the host; equal to the one-piece host histogram."""
    G_row, S, G_col = lattice_factors(m, n_cols, ranks)
    X = np.dot(np.dot(G_row, S), G_col.T)
    e = np.unique(X)
    assert e.size > MAX_EDGES and (n_distinct is None or e.size == n_distinct), e.size
    ex = exclusion_mask(pattern, m, n_cols)
    tg = target_mask(m, n_cols)
    want, want_t = host_hist(X, e, ex, tg)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    xl, tl = lists_of(ex), lists_of(tg)

    def blocks(step, targets=True):
        def walk():
            for (A, x), (_, t) in zip(blocks_of(G_row, xl, step)(), blocks_of(G_row, tl, step)()):
                yield A, x, t if targets else None
        return walk
    walks = []
    one = DeviceCompleter.hist

    def counting(self, *a, **kw):
        walks.append(1)
        return one(self, *a, **kw)
    DeviceCompleter.hist = counting
    try:
        counts, tcounts, cands = comp.histogram(blocks(8192), e)
    finally:
        DeviceCompleter.hist = one
    assert len(walks) == -(-e.size // MAX_EDGES)
    what = 'hist walks %s %dx%d' % (dtype, m, n_cols)
    assert counts.dtype == np.int64 and np.array_equal(counts, want) and np.array_equal(tcounts, want_t) and cands == want.sum(), what
    counts, tcounts, cands = comp.histogram(blocks(64, targets=False), e, col_splits=3)
    assert tcounts is None and np.array_equal(counts, want), what + ' in row blocks of 64, no targets'
    fit, rel = model(G_row, S, G_col)
    got = fit.complete_histogram(rel, e, exclude=sparse_of(ex), targets=sparse_of(tg), dtype=dtype)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want_t), what + ' complete_histogram'


# ---- 2. P6 and P7 ------------------------------------------------------------------------------------------------------------
def p6_case(dtype, m, n_cols, ranks, pattern='edges', split_pairs=((0, 3), (1, 2)), signed=False):
    """P6: the bins above t sum to *n_found of skf_complete_above (count only) at thr = edges[t] in every row, for t at both ends
    and a sample in between, for pairs (col_splits of hist, col_splits of above), also with the rows cut into blocks of 64."""
    G_row, S, G_col = factors_of(m, n_cols, ranks, signed)
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    ex = exclusion_mask(pattern, m, n_cols)
    e = edge_sets(X, dtype, signed)['every distinct score']
    ts = np.unique(np.concatenate([[0, e.size - 1], np.linspace(0, e.size - 1, 7).astype(np.int64)]))
    raw = Raw(dtype, H, G_col)
    xl = None if ex is None else lists_of(ex)
    cut = [(Raw(dtype, A, G_col), x) for A, x in blocks_of(H, xl, 64)()]
    what = 'hist P6 %s m %d n_cols %d ranks %r %s' % (dtype, m, n_cols, ranks, pattern)
    for sh, sa in split_pairs:
        whole = at_or_above(raw_hist(raw, e, ex, col_splits=sh)[0])
        parts = np.zeros(e.size + 1, dtype=np.int64)
        for r, x in cut:
            parts += raw_hist(r, e, xlists=x, col_splits=sh)[0]
        assert at_or_above(parts) == whole, '%s: the row blocks of 64 do not sum to the whole (splits %d)' % (what, sh)
        for t in ts:
            found = int(raw_above(raw, np.full(m, e[t]), ex, col_splits=sa, mode='count')[0][-1])
            assert whole[t] == found, '%s splits %d / %d: %d at or above edge %d, above() finds %d' % (what, sh, sa, whole[t], t, found)
            in_blocks = sum(int(raw_above(r, np.full(r.m, e[t]), xlists=x, col_splits=sa, mode='count')[0][-1]) for r, x in cut)
            assert in_blocks == found, what + ': above() in row blocks'


def p7_case(dtype, m, n_cols, ranks, pattern='edges', signed=False):
    """P7: a counted target lands in the bin of its out_val of skf_complete_ranks; excluded and NaN targets are counted nowhere."""
    G_row, S, G_col = factors_of(m, n_cols, ranks, signed)
    H = np.dot(G_row, S)
    H[m // 2, 0] = np.nan                                            # a row of NaN scores, with targets
    raw = Raw(dtype, H, G_col)
    ex = exclusion_mask(pattern, m, n_cols)
    tg = target_mask(m, n_cols)
    tg[m // 2, :3] = True
    tl = lists_of(tg)
    rank, val = raw_ranks(raw, tl, ex)
    val = val.astype(np.float64)
    counted = ~np.isnan(val) & (True if ex is None else ~ex[rows_of(tl), tl[1]])
    assert (rank[np.isnan(val)] == -1).all() and np.isnan(val).sum() >= 3 and 0 < counted.sum() < counted.size
    with np.errstate(invalid='ignore'):
        X = np.dot(H, G_col.T)
    for name, e in edge_sets(X, dtype, signed).items():
        want = np.bincount(np.searchsorted(e, val[counted], side='right'), minlength=e.size + 1)
        for s in (0, 2):
            got = raw_hist(raw, e, ex, tg, col_splits=s)[1]
            assert np.array_equal(got, want), 'hist P7 %s m %d n_cols %d %s, %s splits %d' % (dtype, m, n_cols, pattern, name, s)


# ---- 3. random cases -------------------------------------------------------------------------------------------------------
def band_check(counts, X64, ok, e, Bm, what):
    """For every edge: #{X64 >= e + B} <= the device's count at or above it <= #{X64 >= e - B}.  Returns the widest band."""
    v = np.sort(X64[ok])
    got = np.array(at_or_above(counts))
    lo = v.size - np.searchsorted(v, e + Bm, side='left')
    hi = v.size - np.searchsorted(v, e - Bm, side='left')
    bad = np.nonzero((got < lo) | (got > hi))[0]
    assert bad.size == 0, '%s: %d at or above edge %d (%.9g), the float64 band is [%d, %d]' % (
        what, got[bad[0]] if bad.size else 0, bad[0] if bad.size else 0, e[bad[0]] if bad.size else 0, lo[bad[0]] if bad.size else 0,
        hi[bad[0]] if bad.size else 0)
    assert counts.sum() == v.size, what + ': not every candidate is counted'
    return int((hi - lo).max())


def random_case(dtype, ranks, m=131, n_cols=997, pattern='heavy', n_edges=64, label=''):
    T_ = NPT[dtype]
    G_row, S, G_col = (x.astype(T_).astype(np.float64) for x in random_factors(m, n_cols, ranks))   # rounded to the scoring type
    X64 = np.dot(np.dot(G_row, S), G_col.T)
    Bm = float(bound(G_row, S, G_col, dtype).max())
    ex = exclusion_mask(pattern, m, n_cols)
    ok = np.ones(X64.shape, dtype=bool) if ex is None else ~ex
    tg = target_mask(m, n_cols) | (np.random.RandomState(3).rand(m, n_cols) < 0.01)
    e = in_type(np.quantile(X64, np.linspace(0.0, 1.0, n_edges)), dtype)
    fit, rel = model(G_row, S, G_col)
    counts, tcounts = fit.complete_histogram(rel, e, exclude=None if ex is None else sparse_of(ex), targets=sparse_of(tg), dtype=dtype)
    what = '%s hist random %s %dx%d ranks %r %s' % (label, dtype, m, n_cols, ranks, pattern)
    wide = band_check(counts, X64, ok, e, Bm, what)
    wide_t = band_check(tcounts, X64, ok & tg, e, Bm, what + ' targets')
    line = '%s: %d edges, B = %.3g, widest band %d of %d candidates, %d of %d targets' % (what, e.size, Bm, wide, ok.sum(), wide_t, (ok & tg).sum())
    print(line)
    DEVIATIONS.append(line)


# ---- 4. NaN and infinities ---------------------------------------------------------------------------------------------------
def nan_inf_case(dtype, m=67, n_cols=203, ranks=(5, 2)):
    G_row, S, G_col = lattice_factors(m, n_cols, ranks)
    S[0] = np.maximum(S[0], 0.125)
    G_row[9, 1] = np.nan                                             # a NaN row
    G_row[4] = 0.0
    G_row[4, 0] = np.inf                                             # row 4: +inf / NaN (inf * 0)
    G_row[11] = 0.0
    G_row[11, 0] = -np.inf                                           # row 11: -inf / NaN
    with np.errstate(invalid='ignore'):
        X = np.dot(np.dot(G_row, S), G_col.T)
    assert np.isnan(X[9]).all() and np.isposinf(X[4]).sum() > 70 and np.isneginf(X[11]).sum() > 70
    ex = exclusion_mask('heavy', m, n_cols)
    assert ex[3].all() and not ex[4].all() and not ex[11].all()
    tg = target_mask(m, n_cols)
    tg[[4, 9, 11], ::5] = True
    fit, rel = model(G_row, S, G_col)
    xs, ts = sparse_of(ex), sparse_of(tg)
    fin = np.unique(X[np.isfinite(X)])
    n_pos, n_neg = int((np.isposinf(X) & ~ex).sum()), int((np.isneginf(X) & ~ex).sum())
    for e in (np.array([-np.inf, fin[fin.size // 2], np.inf]), np.array([fin[1], fin[-2]]), np.array([np.inf]), np.array([-np.inf])):
        want, want_t = host_hist(X, e, ex, tg)
        for step in (8192, 3):
            got, got_t = fit.complete_histogram(rel, e, exclude=xs, targets=ts, dtype=dtype, block_rows=step)
            assert np.array_equal(got, want) and np.array_equal(got_t, want_t), 'hist NaN / inf %s edges %r' % (dtype, e)
        assert want[-1] >= n_pos and (want[-1] == n_pos) == bool(e[-1] == np.inf), '+inf scores land in the last bin'
        assert (want[0] == 0 and want[1] >= n_neg) if e[0] == -np.inf else want[0] >= n_neg, '-inf scores land in bin 0 unless edges[0] = -inf'
    e = np.array([-np.inf, 0.0, np.inf])
    for rows in ([9, 9], [3], [9, 3]):                               # NaN scores, every column excluded: nothing is added
        got, got_t = fit.complete_histogram(rel, e, rows=rows, exclude=xs, targets=ts, dtype=dtype)
        assert not got.any() and not got_t.any(), rows
    curve = fit.complete_curve(rel, ts, edges=e, rows=[9, 3], exclude=xs, dtype=dtype)
    assert curve.n_candidates == 0 and curve.n_positives == 0 and curve.n_positives_given == int(tg[9].sum() + tg[3].sum())
    assert np.isnan(curve.auroc).all() and np.isnan(curve.precision).all() and np.isnan(curve.recall).all() and np.isnan(curve.fpr).all()


# ---- 5. independence -----------------------------------------------------------------------------------------------------------
def independence_case(dtype, m=131, n_cols=203, ranks=(20, 64), pattern='edges', n_edges=100):
    G_row, S, G_col = random_factors(m, n_cols, ranks)
    ex = exclusion_mask(pattern, m, n_cols)
    tg = target_mask(m, n_cols)
    xl, tl = lists_of(ex), lists_of(tg)
    e = np.quantile(np.dot(np.dot(G_row, S), G_col.T), np.linspace(0, 1, n_edges))
    fit, rel = model(G_row, S, G_col)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    first = None
    for step in (64, 8192):
        got = fit.complete_histogram(rel, e, exclude=sparse_of(ex), targets=sparse_of(tg), dtype=dtype, block_rows=step)
        first = first or (got[0].tobytes(), got[1].tobytes())
        assert (got[0].tobytes(), got[1].tobytes()) == first, 'complete_histogram %s: block_rows %d changes the counts' % (dtype, step)
        for s in SPLITS:
            walk = lambda: ((A, x, t) for (A, x), (_, t) in zip(blocks_of(G_row, xl, step)(), blocks_of(G_row, tl, step)()))
            c, t, _ = comp.histogram(walk, e, col_splits=s)
            assert (c.tobytes(), t.tobytes()) == first, 'histogram %s: block_rows %d col_splits %d changes the counts' % (dtype, step, s)
    return first


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def refusals_without_device(lib, ptr):
    """Everything refused before any HIP call (`ptr`: any non-null, 256-byte aligned address; it is never dereferenced)."""
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    need = C.c_size_t()
    assert lib.skf_complete_hist_workspace_bytes(nat.SKF_F32, 67, 203, 100, 0, C.byref(need)) == 0
    nb = need.value
    assert 256 <= nb < 4096, 'flag words: nothing of the size of the relation, the targets or the edges'

    def hist(dtype=nat.SKF_F32, H=ptr, Gc=ptr, c=8, ldh=8, ldg=8, edges=ptr, n_edges=16, xp=None, xi=None, tp=ptr, ti=ptr, n_targets=100,
             hist=ptr, hist_tgt=ptr, ws=ptr, ws_bytes=nb, splits=0, m=67, n_cols=203):
        return lib.skf_complete_hist(dtype, H, ldh, m, Gc, ldg, n_cols, c, edges, n_edges, xp, xi, tp, ti, n_targets, hist, hist_tgt, splits,
                                     ws, ws_bytes, None)
    for kw in (dict(dtype=nat.SKF_BF16), dict(dtype=7), dict(m=-1), dict(m=2 ** 31), dict(n_cols=-1), dict(n_cols=2 ** 31), dict(c=0),
               dict(c=1025), dict(H=None), dict(Gc=None), dict(ldh=7), dict(ldg=7), dict(splits=-1), dict(splits=33), dict(xp=ptr),
               dict(xi=ptr), dict(n_edges=0), dict(n_edges=-1), dict(n_edges=2048), dict(edges=None), dict(hist=None), dict(tp=None),
               dict(ti=None), dict(hist_tgt=None), dict(tp=None, ti=None), dict(tp=None, hist_tgt=None), dict(ti=None, hist_tgt=None),
               dict(n_targets=-1), dict(tp=None, ti=None, hist_tgt=None, n_targets=100)):
        assert hist(**kw) == INV, kw
        assert b'skf_complete_hist' in lib.skf_last_error(), kw
    assert hist(ws_bytes=nb - 1) == WS and hist(ws=None) == WS and hist(ws=ptr + 8) == WS
    for kw in (dict(splits=33), dict(splits=-1), dict(m=-1), dict(m=2 ** 31), dict(n_cols=2 ** 31), dict(dtype=nat.SKF_BF16), dict(n_targets=-1)):
        assert lib.skf_complete_hist_workspace_bytes(kw.get('dtype', nat.SKF_F32), kw.get('m', 67), kw.get('n_cols', 203),
                                                     kw.get('n_targets', 100), kw.get('splits', 0), C.byref(need)) == INV, kw
    assert lib.skf_complete_hist_workspace_bytes(nat.SKF_F32, 67, 203, 100, 0, None) == INV
    assert lib.skf_complete_hist_workspace_bytes(nat.SKF_F64, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 40, 32, C.byref(need)) == 0 and need.value == nb


def refusals_case(dtype='f64'):
    """Every refusal leaves both histograms and the memory behind them as they were; what is refused before any HIP call
    leaves the workspace as it was and launches nothing; what the device finds is refused after the validation launches alone
    -- one per list given and one for the edges."""
    rt = nat.get_runtime()
    keep = rt.mem.empty(16384)
    refusals_without_device(rt.lib, keep.ptr)
    m, n_cols = 37, 70
    G_row, S, G_col = lattice_factors(m, n_cols, (5, 7))
    H = np.dot(G_row, S)
    raw = Raw(dtype, H, G_col)
    ex = exclusion_mask('edges', m, n_cols)
    xl = lists_of(ex)
    tg = target_mask(m, n_cols)
    tg[4, :5] = True
    tl = lists_of(tg)
    e = np.unique(np.dot(H, G_col.T))[::7]
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    start = np.arange(e.size + 1, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    start_t = start + np.uint64(11)
    nb = hist_workspace(raw, len(tl[1]))

    def refused(want, message, launches, *args, **kw):
        before = launch_count()
        s0, s1 = start[:len(args[0]) + 1], start_t[:len(args[0]) + 1]
        rc, h, t, intact, clean = call_hist(raw, *args, start=s0, start_tgt=s1, **kw)
        what = '%r %r' % (message, kw)
        assert rc == want and message in rt.lib.skf_last_error(), '%s: status %d, %r' % (what, rc, rt.lib.skf_last_error())
        assert np.array_equal(h, s0) and np.array_equal(t, s1) and intact, what + ': a histogram was written'
        assert launch_count() - before == launches, what + ': %d launches' % (launch_count() - before)
        assert clean or launches, what + ': the workspace was written'

    for want, over in ((INV, dict(dtype=nat.SKF_BF16)), (INV, dict(m=-1)), (INV, dict(m=2 ** 31)), (INV, dict(n_cols=-1)),
                       (INV, dict(n_cols=2 ** 31)), (INV, dict(c=0)), (INV, dict(c=1025)), (INV, dict(H=None)), (INV, dict(Gc=None)),
                       (INV, dict(ldh=raw.c - 1)), (INV, dict(ldg=raw.c - 1)), (INV, dict(splits=-1)), (INV, dict(splits=33)),
                       (INV, dict(xp=None)), (INV, dict(xi=None)), (INV, dict(tp=None)), (INV, dict(ti=None)), (INV, dict(hist_tgt=None)),
                       (INV, dict(tp=None, ti=None)), (INV, dict(n_edges=0)), (INV, dict(n_edges=2048)), (INV, dict(edge_ptr=None)),
                       (INV, dict(hist=None)), (INV, dict(n_targets=-1)), (WS, dict(ws_bytes=nb - 1)), (WS, dict(ws=None))):
        refused(want, b'skf_complete_hist', 0, e, xl, tl, **over)
    ws = rt.mem.empty(nb + 256)
    refused(WS, b'aligned', 0, e, xl, tl, ws=ws.ptr + 8, ws_bytes=nb)
    # found on the device, by the validation alone
    desc, nan = e.copy(), e.copy()
    desc[3], desc[4] = e[4], e[3]
    nan[e.size // 2] = np.nan
    for s in (1, 2):
        refused(INV, b'edges', 3, desc, xl, tl, col_splits=s)
        refused(INV, b'edges', 3, nan, xl, tl, col_splits=s)
        refused(INV, b'edges', 1, desc[3:5], col_splits=s)
        refused(INV, b'edges', 1, np.array([np.nan]), col_splits=s)
        for name, (p, i, n) in defective_lists(xl[0], xl[1], m, n_cols).items():
            if name in ('count does not match indptr[m]', 'indptr does not end at its count'):
                continue                                         # (the exclusion lists carry no count but indptr[m])
            before = launch_count()
            rc, h, t, intact, _ = call_hist(raw, e, (p, i), tl, col_splits=s, start=start, start_tgt=start_t)
            assert rc == INV and b'exclusion lists' in rt.lib.skf_last_error(), 'exclusion: ' + name
            assert np.array_equal(h, start) and np.array_equal(t, start_t) and intact, 'exclusion: %s: a histogram was written' % name
            assert launch_count() - before <= 3, 'exclusion: %s: something ran after the validation' % name
        for name, (p, i, n) in defective_lists(tl[0], tl[1], m, n_cols).items():
            refused(INV, b'target lists', 3, e, xl, (p, i), col_splits=s, n_targets=n)
            refused(INV, b'target lists', 2, e, None, (p, i), col_splits=s, n_targets=n)
    refused(INV, b'target lists', 3, e, xl, tl, n_targets=len(tl[1]) + 1)
    got, got_t = raw_hist(raw, e, ex, tg, start=start, start_tgt=start_t)       # everything as it was is accepted
    assert int(got.sum()) == int((~ex).sum()) and int(got_t.sum()) == int((tg & ~ex).sum())


def python_refusals_case():
    """Every DataFusionError / ValueError of the Python layers, before anything runs."""
    import scipy.sparse
    from skfusion_amd.fusion.base import DataFusionError
    m, n_cols = 12, 9
    G_row, S, G_col = lattice_factors(m, n_cols, (5, 7))
    fit, rel = model(G_row, S, G_col)
    pos = sparse_of(target_mask(m, n_cols))
    for method, args in ((fit.complete_histogram, ()), (fit.complete_curve, (pos,))):
        for bad in (np.zeros((2, 2)), np.zeros(0), 0.5, np.array(['a', 'b']), np.array([1j]), [0.0, np.nan], [1.0, 0.5], [0.0, 1.0, 0.5]):
            with pytest.raises(DataFusionError, match='edges'):
                method(rel, *args, edges=bad) if args else method(rel, bad)
        with pytest.raises(DataFusionError, match='rows'):
            method(rel, *args, edges=[0.5], rows=[m]) if args else method(rel, [0.5], rows=[m])
        with pytest.raises(DataFusionError, match='shape'):
            method(rel, *args, edges=[0.5], exclude=scipy.sparse.csr_matrix((m, n_cols + 1))) if args else \
                method(rel, [0.5], exclude=scipy.sparse.csr_matrix((m, n_cols + 1)))
    with pytest.raises(DataFusionError, match='edges'):
        fit.complete_histogram(rel, None)
    with pytest.raises(DataFusionError, match='targets has shape'):
        fit.complete_histogram(rel, [0.5], targets=scipy.sparse.csr_matrix((m + 1, n_cols)))
    with pytest.raises(DataFusionError, match='targets must be a scipy.sparse matrix'):
        fit.complete_histogram(rel, [0.5], targets=np.zeros((m, n_cols)))
    with pytest.raises(DataFusionError, match='positives has shape'):
        fit.complete_curve(rel, scipy.sparse.csr_matrix((m, n_cols - 1)))
    with pytest.raises(DataFusionError, match='positives must be a scipy.sparse matrix'):
        fit.complete_curve(rel, None)
    with pytest.raises(DataFusionError, match='n_edges'):
        fit.complete_curve(rel, pos, n_edges=0)
    post_fit, post = model(G_row, S, G_col, postprocessor=lambda x: np.clip(x, 0.0, 1.0))
    with pytest.raises(DataFusionError, match='postprocessor'):
        post_fit.complete_histogram(post, [0.5])
    with pytest.raises(DataFusionError, match='postprocessor'):
        post_fit.complete_curve(post, pos)
    # the device layer
    comp = DeviceCompleter(S, G_col, dtype='f32')
    blocks = lambda: iter([(G_row, None, None)])
    for bad in (np.zeros((2, 2)), np.zeros(0), [0.0, np.nan], [1.0, 0.5]):
        with pytest.raises(ValueError, match='edges'):
            comp.histogram(blocks, bad)
    mem = comp.rt.mem
    e, h = mem.from_host(np.zeros(4, dtype=np.float32)), mem.from_host(np.zeros(5, dtype=np.uint64))
    with pytest.raises(ValueError, match='hist'):
        comp.hist(G_row, e, mem.from_host(np.zeros(4, dtype=np.uint64)))
    with pytest.raises(ValueError, match='come together'):
        comp.hist(G_row, e, h, targets=lists_of(target_mask(m, n_cols)))
    with pytest.raises(ValueError, match='come together'):
        comp.hist(G_row, e, h, hist_targets=h)
    with pytest.raises(ValueError, match='hist'):
        comp.hist(G_row, e, h, targets=lists_of(target_mask(m, n_cols)), hist_targets=mem.from_host(np.zeros(4, dtype=np.uint64)))
    with pytest.raises(ValueError, match='targets: indptr'):
        comp.hist(G_row, e, h, targets=(np.zeros(m, dtype=np.int64), np.zeros(0, dtype=np.int32)), hist_targets=h)
    with pytest.raises(ValueError, match='all or none'):
        comp.histogram(lambda: iter([(G_row, None, None), (G_row, None, lists_of(target_mask(m, n_cols)))]), [0.5])


# ---- 7. public API and the curve -------------------------------------------------------------------------------------------
def host_curve(X, e, ex, pos):
    """(predicted, true_positives, n_candidates, n_positives, the mid-rank AUROC as a Fraction or None) on the float64 scores."""
    ok = ~np.isnan(X)
    if ex is not None:
        ok &= ~ex
    s, y = X[ok], pos[ok]
    predicted = np.array([(s >= t).sum() for t in e], dtype=np.int64)
    tp = np.array([(s[y] >= t).sum() for t in e], dtype=np.int64)
    P, N = int(y.sum()), int((~y).sum())
    mid = None
    if P and N:
        neg = np.sort(s[~y])
        twice = sum(int(np.searchsorted(neg, v, side='left')) + int(np.searchsorted(neg, v, side='right')) for v in s[y])
        mid = fractions.Fraction(twice, 2 * P * N)                  # every negative below counts 1, every equal one 1/2
    return predicted, tp, s.size, P, mid


def counts_of(curve):
    """The two histograms a CompletionCurve was read from."""
    c = np.concatenate([[curve.n_candidates - curve.predicted[0]], -np.diff(curve.predicted), [curve.predicted[-1]]])
    t = np.concatenate([[curve.n_positives - curve.true_positives[0]], -np.diff(curve.true_positives), [curve.true_positives[-1]]])
    return c, t


def check_curve(curve, X, e, ex, pos, given, what):
    """A curve on edges = every distinct score of X against the host's; `given`: the stored positives of the rows asked for."""
    from skfusion_amd.fusion._completion import auroc_bounds
    predicted, tp, cands, P, mid = host_curve(X, e, ex, pos)
    assert np.array_equal(curve.thresholds, e) and curve.thresholds.dtype == np.float64, what
    assert curve.predicted.dtype == np.int64 and np.array_equal(curve.predicted, predicted), what + ': predicted'
    assert curve.true_positives.dtype == np.int64 and np.array_equal(curve.true_positives, tp), what + ': true_positives'
    assert (curve.n_candidates, curve.n_positives, curve.n_positives_given) == (cands, P, given), what
    N = cands - P
    some = predicted > 0
    # one division and one multiplication in float64: two roundings
    assert (np.abs(curve.precision[some] * predicted[some] - tp[some]) <= 2.0 ** -51 * tp[some]).all() and np.isnan(curve.precision[~some]).all()
    assert np.array_equal(curve.recall, tp / float(P)) and np.array_equal(curve.fpr, (predicted - tp) / float(N)), what
    lo, hi = auroc_bounds(*counts_of(curve))
    assert (lo + hi) / 2 == mid, '%s: (lo + hi) / 2 = %s, the mid-rank AUROC %s' % (what, (lo + hi) / 2, mid)
    assert curve.auroc == (float(lo), float(hi)) and 0 <= lo <= hi <= 1, what


def curve_case(dtype, m=67, n_cols=203, ranks=(5, 7), pattern='edges', signed=False):
    """complete_curve on lattice factors with edges = every distinct score: counts and the mid-rank AUROC exactly."""
    G_row, S, G_col = factors_of(m, n_cols, ranks, signed)
    X = np.dot(np.dot(G_row, S), G_col.T)
    e = np.unique(X)
    ex = exclusion_mask(pattern, m, n_cols)
    pos = (np.random.RandomState(5).rand(m, n_cols) < 0.02 + 0.2 * (X > np.median(X))) | target_mask(m, n_cols)
    assert ex is None or (ex & pos).any()
    fit, rel = model(G_row, S, G_col)
    xs = None if ex is None else sparse_of(ex)
    what = 'curve %s m %d n_cols %d ranks %r %s' % (dtype, m, n_cols, ranks, pattern)
    for step in (8192, 64):
        check_curve(fit.complete_curve(rel, sparse_of(pos), edges=e, exclude=xs, dtype=dtype, block_rows=step), X, e, ex, pos, int(pos.sum()), what)


def default_edges_case(dtype='f64', m=131, n_cols=203, ranks=(20, 64), pattern='edges'):
    """Default edges on random factors: the AUROC of the float64 scores lies in [lo, hi].  The bins are read from the device's
    scores, the truth from X64: the two orders differ only for pairs closer than the rounding of a score (relative 1e-15 here,
    c_i + c_j + 5 roundings of 2^-53), and a bound moves by 1 / (P N) only when such a pair is a positive and a negative on
    either side of an edge; with some 10^6 (positive, negative) pairs spread over a range of 10^-2 that has a probability below
    10^-6, and the case runs in f64 alone.  With fewer edges than positives the truth is strictly inside."""
    from skfusion_amd.fusion._completion import auroc_bounds
    G_row, S, G_col = random_factors(m, n_cols, ranks)
    X64 = np.dot(np.dot(G_row, S), G_col.T)
    ex = exclusion_mask(pattern, m, n_cols)
    pos = np.random.RandomState(6).rand(m, n_cols) < 0.01 + 0.03 * (X64 > np.quantile(X64, 0.7))
    fit, rel = model(G_row, S, G_col)
    truth = host_curve(X64, [], ex, pos)[4]
    P = int((pos & ~ex).sum())
    assert truth is not None and 0.5 < truth < 1 and P > 300
    widths = []
    for n_edges in (2047, 16, 1):
        curve = fit.complete_curve(rel, sparse_of(pos), n_edges=n_edges, exclude=sparse_of(ex), dtype=dtype)
        lo, hi = auroc_bounds(*counts_of(curve))
        assert curve.auroc == (float(lo), float(hi)) and lo <= truth <= hi, 'default edges %d: AUROC %.12f outside [%.12f, %.12f]' % (
            n_edges, float(truth), float(lo), float(hi))
        assert 1 <= curve.thresholds.size <= n_edges and (np.diff(curve.thresholds) > 0).all()
        assert curve.n_positives == P and curve.n_positives_given == int(pos.sum()) and curve.n_candidates == int((~ex).sum())
        widths.append(hi - lo)
        print('default edges: n_edges %d -> %d thresholds, AUROC in [%.6f, %.6f], float64 %.6f' % (n_edges, curve.thresholds.size, lo, hi, truth))
    assert widths[0] < widths[1] < widths[2] and widths[0] < fractions.Fraction(1, 100), 'more edges must narrow the bounds'
    assert lo < truth < hi


def _pattern(data):
    """Boolean [n_i, n_j] of the stored entries of a scipy.sparse matrix, without expanding it through scipy."""
    coo = data.tocoo()
    out = np.zeros(data.shape, dtype=bool)
    out[coo.row, coo.col] = True
    return out


def api_case(kind, monkeypatch):
    """The fitted models of above_cases.api_case ('dfmc-masked' with exclude='known', 'dfmf-csr') with factors rounded to a
    coarse lattice, so that the host's bins are exact; complete(), _reconstruct() and toarray() raise."""
    import above_cases as AC
    from skfusion_amd.fusion.base import FusionFit
    fuser = AC.api_case(kind, monkeypatch)                           # (sparse matrices can no longer be expanded)
    rel = list(fuser.fusion_graph.relations)[0]
    users, movies = rel.row_type, rel.col_type
    for t in (users, movies):                                        # multiples of 1/64: every partial sum is exact
        fuser.factors_[t] = [np.round(np.asarray(G) * 64) / 64 for G in fuser.factors_[t]]
    fuser.backbones_[rel] = [np.round(np.asarray(S) * 64) / 64 for S in fuser.backbones_[rel]]
    X = np.dot(np.dot(fuser.factor(users), fuser.backbone(rel)), fuser.factor(movies).T)
    n_i, n_j = X.shape
    data = rel.data
    known = ~np.ma.getmaskarray(data) if np.ma.isMaskedArray(data) else _pattern(data)
    pos = np.random.RandomState(8).rand(n_i, n_j) < 0.1 + 0.3 * (X > np.median(X))
    assert (pos & known).any() and (pos & ~known).any()
    ps = sparse_of(pos)
    e = np.unique(X)
    what = 'api hist %s' % kind

    def boom(*a, **kw):
        raise AssertionError('the dense reconstruction was formed')
    monkeypatch.setattr(FusionFit, 'complete', boom)
    monkeypatch.setattr(FusionFit, '_reconstruct', boom)
    for exclude, ex in ((None, None), ('known', known)):
        want, want_t = host_hist(X, e, ex, pos)
        got = fuser.complete_histogram(rel, e, exclude=exclude)
        assert got.dtype == np.int64 and np.array_equal(got, want), what
        for fmt in (ps, ps.tocsc(), ps.tocoo()):
            got, got_t = fuser.complete_histogram(rel, e, exclude=exclude, targets=fmt, block_rows=7)
            assert np.array_equal(got, want) and np.array_equal(got_t, want_t), what + ' targets'
        check_curve(fuser.complete_curve(rel, ps, edges=e, exclude=exclude, block_rows=7), X, e, ex, pos, int(pos.sum()), what)
    # the size complete_above returns at a threshold is the sum of the bins above its edge
    t = e.size // 3
    assert fuser.complete_above(rel, e[t], exclude='known').nnz == int(host_hist(X, e, known)[0][t + 1:].sum())
    # rows in arbitrary order with a duplicate: a row listed twice is two rows
    rows = np.array([17, 3, 3, 39, 0])
    want, want_t = host_hist(X[rows], e, known[rows], pos[rows])
    got, got_t = fuser.complete_histogram(rel, e, rows=rows, exclude='known', targets=ps, block_rows=2)
    assert np.array_equal(got, want) and np.array_equal(got_t, want_t), what + ' rows='
    check_curve(fuser.complete_curve(rel, ps, edges=e, rows=rows, exclude='known', block_rows=2), X[rows], e, known[rows], pos[rows],
                int(pos[rows].sum()), what + ' rows=')
    # no rows; integer edges; a single edge
    got, got_t = fuser.complete_histogram(rel, e, rows=np.zeros(0, dtype=int), targets=ps)
    assert got.shape == got_t.shape == (e.size + 1,) and not got.any() and not got_t.any()
    assert np.array_equal(fuser.complete_histogram(rel, [0, 1]), host_hist(X, [0.0, 1.0])[0])
    assert np.array_equal(fuser.complete_histogram(rel, e[5:6], exclude='known'), host_hist(X, e[5:6], known)[0])
    # edges are cast to the scoring type: 'bf16' scores on the f32 masters, and a cast that merges two edges leaves an empty bin
    a = fuser.complete_histogram(rel, e, exclude='known', targets=ps, dtype='f32')
    b = fuser.complete_histogram(rel, e, exclude='known', targets=ps, dtype='bf16')
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].sum() == (~known).sum()
    close = np.array([e[4], e[4] + 1e-12, e[9]])
    assert np.float32(close[0]) == np.float32(close[1])
    merged = fuser.complete_histogram(rel, close, dtype='f32')
    assert merged[1] == 0 and np.array_equal(merged, host_hist(X, in_type(close, 'f32'))[0])
    assert np.array_equal(fuser.complete_histogram(rel, close, dtype='f64'), host_hist(X, close)[0])


def api_runs_case():
    """n_run = 2 and run=None: a generator over the runs, each equal to the explicit run."""
    import types
    import known_csr_api_cases as KA
    from skfusion_amd.fusion import Dfmc
    _, ma = KA.ratings(40, 30, 0.2, 11)
    g, users, movies = KA.graph(ma, ranks=(5, 4, 3))
    fuser = KA.fit(Dfmc, g, max_iter=3, init_type='random', random_state=0, dtype='f64', n_run=2)
    rel = list(g.relations)[0]
    e = np.linspace(0.0, 1.0, 33)
    pos = sparse_of(np.random.RandomState(9).rand(40, 30) < 0.2)
    out, curves = fuser.complete_histogram(rel, e, exclude='known', targets=pos), fuser.complete_curve(rel, pos, exclude='known')
    assert isinstance(out, types.GeneratorType) and isinstance(curves, types.GeneratorType)
    out, curves = list(out), list(curves)
    assert len(out) == len(curves) == 2
    for r in range(2):
        one = fuser.complete_histogram(rel, e, exclude='known', targets=pos, run=r)
        assert np.array_equal(out[r][0], one[0]) and np.array_equal(out[r][1], one[1])
        c = fuser.complete_curve(rel, pos, exclude='known', run=r)
        assert np.array_equal(curves[r].thresholds, c.thresholds) and np.array_equal(curves[r].predicted, c.predicted) and curves[r].auroc == c.auroc
    assert not np.array_equal(out[0][0], out[1][0])
