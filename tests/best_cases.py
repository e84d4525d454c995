"""The n best pairs of a whole relation without the dense reconstruction (csrc/skf_complete.h complete_digits_kernel,
skf_complete_digits, _engine.DeviceCompleter.digits / kth, FusionFit.complete_kth / complete_best) -- the SAME cases on the
host emulator (small) and on the GPU.  The yardstick is host NumPy in float64 on factors rounded to the scoring type: the
host's answer is the first n of the admissible, non-NaN pairs in a stable sort by (-score, row, column).

  1. exact cases (lattice factors, a signed variant among them: every partial sum exact): threshold, counts and the matrix
     index for index and bit for bit, whatever col_splits, block_rows and ties.
  2. the raw operator: every pass of a selection is np.bincount of the host's keys; added to, never cleared; sentinels; refusals.
  3. P3 against skf_complete_above, a single row against complete_topk, returned pairs against complete_ranks.
  4. random cases under the derived bound b = complete_cases.bound: with T the device's threshold and B = max b exactly n
     entries, every value within b, every admissible pair with X64 > T + B present, every pair with X64 < T - B absent; the
     undecided band |X64 - T| <= 2 B holds at most 0.1 % of the admissible pairs.
  5. NaN and infinities, 6. independence of block_rows / col_splits / the 'bf16' name, 7. the public API."""
import ctypes as C

import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DeviceCompleter, digit_walk
from complete_cases import NPT, Raw, bound, exclusion_mask, lattice_factors, lists_of, random_factors
from above_cases import seam_mask

SPLITS = (0, 1, 2, 3, 32)
PAD = 5                                          # sentinel words behind the histogram
SENT = np.uint64(0x5A5A5A5A5A5A5A5A)
PLAN = {'f32': (11, 11, 10), 'bf16': (11, 11, 10), 'f64': (11, 11, 11, 11, 11, 9)}
DEVIATIONS = []                                  # lines of the random cases (the GPU module prints them at the end)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def signed_lattice_factors(m, n_cols, ranks, seed=0):
    """lattice_factors with every odd row of the row factor negated: the sums stay exact, the scores of those rows are
    negative or zero -- the other branch of the key, which the non-negative lattices never take."""
    G_row, S, G_col = lattice_factors(m, n_cols, ranks, seed)
    G_row = G_row.copy()
    G_row[1::2] *= -1.0
    return G_row, S, G_col


def model(G_row, S, G_col, n_run=1, data=None, postprocessor=None):
    """A FusionFit that holds the given factors (what a fuser leaves behind), and its one relation."""
    import scipy.sparse
    from skfusion_amd.fusion import FusionGraph, ObjectType, Relation
    from skfusion_amd.fusion.base import FusionFit
    a, b = ObjectType('rows', G_row.shape[1]), ObjectType('cols', G_col.shape[1])
    if data is None:
        data = scipy.sparse.csr_matrix((G_row.shape[0], G_col.shape[0]))
    rel = Relation(data, a, b, **({'postprocessor': postprocessor} if postprocessor else {}))
    fit = FusionFit()
    fit.fusion_graph = FusionGraph([rel])
    fit.n_run = n_run
    fit.factors_[a] = [G_row] * n_run
    fit.factors_[b] = [G_col] * n_run
    fit.backbones_[rel] = [S] * n_run
    return fit, rel


def sparse_of(ex):
    import scipy.sparse
    r, c = np.nonzero(ex)
    return scipy.sparse.csr_matrix((np.ones(r.size), (r, c)), shape=ex.shape)


# ---- the host's answer ------------------------------------------------------------------------------------------------------
def host_order(X, ex=None):
    """(rows, cols, values) of every candidate -- admissible, not NaN -- in the total order: a stable sort by -score of the
    pairs in (row, column) order."""
    ok = ~np.isnan(X)
    if ex is not None:
        ok &= ~ex
    r, c = np.nonzero(ok)
    o = np.argsort(-X[r, c], kind='stable')
    return r[o], c[o], X[r[o], c[o]]


def host_kth(order, n):
    """(T, n_greater, n_equal, n_candidates) of the definition."""
    v = order[2]
    if v.size == 0:
        return np.nan, 0, 0, 0
    T = v[min(n, v.size) - 1]
    return T, int((v > T).sum()), int((v == T).sum()), int(v.size)


def host_best(order, n, shape, ties='first'):
    """(indptr, indices, values) of the first n pairs of the order (ties='all': and every further pair equal to the n-th)."""
    r, c, v = order
    T, g, e, cands = host_kth(order, n)
    take = 0 if n == 0 or cands == 0 else (g + e if ties == 'all' else min(n, cands))
    r, c, v = r[:take], c[:take], v[:take]
    o = np.lexsort((c, r))
    indptr = np.zeros(shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=shape[0]), out=indptr[1:])
    return indptr, c[o].astype(np.int32), v[o]


def host_keys(values, T):
    """The order-preserving keys of the definition on the host (uint64): u = bits of (value + 0) in the scoring type; a set
    sign bit flips every bit, a clear one is set."""
    bits = 8 * np.dtype(T).itemsize
    u = (np.asarray(values).astype(T) + T(0)).view('u%d' % (bits // 8)).astype(np.uint64)
    sign = np.uint64(1 << (bits - 1))
    return np.where((u >> np.uint64(bits - 1)) == 1, ~u & np.uint64((1 << bits) - 1), u | sign)


def same_kth(got, want, what):
    assert got[1:] == want[1:], '%s: (n_greater, n_equal, n_candidates) %r, the host %r' % (what, got[1:], want[1:])
    assert np.array_equal(np.float64(got[0]), np.float64(want[0]), equal_nan=True), '%s: threshold %r, the host %r' % (what, got[0], want[0])


def same_csr(got, want, what):
    import scipy.sparse
    assert scipy.sparse.isspmatrix_csr(got) and got.dtype == np.float64 and got.has_sorted_indices, what
    assert np.array_equal(got.indptr, want[0]), what + ': indptr differs from the host'
    assert np.array_equal(got.indices, want[1]), what + ': indices differ from the host'
    assert got.data.tobytes() == np.asarray(want[2], dtype=np.float64).tobytes(), what + ': values differ from the host scores'


def csr_bytes(M):
    return M.indptr.astype(np.int64).tobytes(), M.indices.astype(np.int32).tobytes(), M.data.tobytes()


def blocks_of(G_row, xl, step):
    """What DeviceCompleter.kth walks: the rows in blocks of `step`, each with its slice of the exclusion lists."""
    def blocks():
        for b0 in range(0, G_row.shape[0], step):
            b1 = min(b0 + step, G_row.shape[0])
            yield G_row[b0:b1], None if xl is None else (xl[0][b0:b1 + 1] - xl[0][b0], xl[1][xl[0][b0]:xl[0][b1]])
    return blocks


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------
def exact_case(dtype, m, n_cols, ranks, signed=False, patterns=('none', 'edges', 'heavy'), ns=(1, 64, 1000, 'all', 'all+5'),
               splits=SPLITS, block_rows=(8192, 64)):
    G_row, S, G_col = (signed_lattice_factors if signed else lattice_factors)(m, n_cols, ranks)
    X = np.dot(np.dot(G_row, S), G_col.T)
    assert np.abs(X).max() * 512 < 2 ** 23 and np.array_equal(X.astype(np.float32).astype(np.float64), X)      # exact in f32
    assert not signed or ((X < 0).any() and (X[1::2] <= 0).all())
    fit, rel = model(G_row, S, G_col)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    ties_seen = 0
    for pattern in patterns:
        ex = exclusion_mask(pattern, m, n_cols)
        xl = None if ex is None else lists_of(ex)
        xs = None if ex is None else sparse_of(ex)
        order = host_order(X, ex)
        cands = order[2].size
        for n in ns:
            n = {'all': cands, 'all+5': cands + 5}.get(n, n)
            what = 'best exact %s m %d n_cols %d ranks %r signed %d %s n %d' % (dtype, m, n_cols, ranks, signed, pattern, n)
            want = host_kth(order, n)
            ties_seen += want[2] > 1 and want[1] + want[2] > n
            for s in splits if n == ns[0] or n == 1000 else splits[:1]:
                same_kth(comp.kth(blocks_of(G_row, xl, 8192), n, col_splits=s), want, '%s kth splits %d' % (what, s))
            same_kth(comp.kth(blocks_of(G_row, xl, 64), n, col_splits=3), want, what + ' kth in row blocks of 64')
            same_kth(fit.complete_kth(rel, n, exclude=xs, dtype=dtype) + (cands,), want, what + ' complete_kth')
            for ties in ('first', 'all'):
                hb = host_best(order, n, X.shape, ties)
                assert ties == 'all' or hb[0][-1] == min(n, cands)
                first = None
                for step in block_rows:
                    got = fit.complete_best(rel, n, exclude=xs, dtype=dtype, ties=ties, block_rows=step)
                    same_csr(got, hb, '%s ties %s block_rows %d' % (what, ties, step))
                    first = first or csr_bytes(got)
                    assert csr_bytes(got) == first, what + ': block_rows changes the bytes'
    return ties_seen


def seam_case(dtype, m=67, n_cols=203, ranks=(5, 7)):
    """The first column of the second of two splits (column 128) against exclusion lists that hold columns 127 and 128, one of
    them or neither (above_cases.seam_mask), with n chosen so that the n-th pair sits in column 127 or 128: two splits, one
    split and the host agree, and the host's answer depends on the seam's entries."""
    seam = 128
    G_row, S, G_col = lattice_factors(m, n_cols, ranks, seed=1)
    X = np.dot(np.dot(G_row, S), G_col.T)
    ex = seam_mask(m, n_cols, seam)
    xl = lists_of(ex)
    order = host_order(X, ex)
    at = np.nonzero((order[1] == seam - 1) | (order[1] == seam))[0]
    assert at.size > 8
    open_seam = ex.copy()
    open_seam[:, seam - 1:seam + 1] = False
    loose = host_order(X, open_seam)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    differs = 0
    for p in at[[0, at.size // 2, at.size - 1]]:
        n = int(p) + 1                                                # the n-th pair lies in the tile at the seam
        want = host_kth(order, n)
        differs += want != host_kth(loose, n)
        for s in (2, 1):
            same_kth(comp.kth(blocks_of(G_row, xl, 8192), n, col_splits=s), want, 'best seam %s n %d splits %d' % (dtype, n, s))
    assert differs, 'the selection does not depend on the seam entries'


# ---- 2. the raw operator ---------------------------------------------------------------------------------------------------
def digits_workspace(raw, col_splits=0):
    need = C.c_size_t()
    raw.rt.call('skf_complete_digits_workspace_bytes', raw.code, raw.m, raw.n_cols, col_splits, C.byref(need))
    return need.value


def call_digits(raw, pfx, pfx_bits, digit_bits, xlists=None, col_splits=0, start=None, **over):
    """skf_complete_digits on the buffers of a complete_cases.Raw: the histogram starts as `start` (default: zeros) with PAD
    sentinel words behind it, the workspace is exactly what the query asks for with 256 sentinel bytes behind it.  `over`
    replaces single arguments (None: a NULL pointer).  Returns (status, histogram as it stands [bins], both sentinels intact)."""
    rt, mem = raw.rt, raw.rt.mem
    bins = 1 << digit_bits if 1 <= digit_bits <= 11 else 2048
    h0 = np.zeros(bins, dtype=np.uint64) if start is None else np.asarray(start, dtype=np.uint64)
    hist = mem.from_host(np.concatenate([h0, np.full(PAD, SENT, dtype=np.uint64)]))
    need = digits_workspace(raw, col_splits)
    ws = mem.from_host(np.full(need + 256, 0x5A, dtype=np.uint8))
    xp = xi = None
    if xlists is not None:
        xp = mem.from_host(np.asarray(xlists[0], dtype=np.int64))
        xi = mem.from_host(np.asarray(xlists[1], dtype=np.int32) if len(xlists[1]) else np.zeros(1, dtype=np.int32))
    a = dict(dtype=raw.code, H=raw.h.ptr, ldh=raw.ldh, m=raw.m, Gc=raw.g.ptr, ldg=raw.ldg, n_cols=raw.n_cols, c=raw.c,
             xp=xp.ptr if xp else None, xi=xi.ptr if xi else None, prefix=pfx, pbits=pfx_bits, dbits=digit_bits, hist=hist.ptr,
             splits=col_splits, ws=ws.ptr, ws_bytes=need)
    assert set(over) <= set(a), over
    a.update(over)
    rc = rt.lib.skf_complete_digits(a['dtype'], a['H'], a['ldh'], a['m'], a['Gc'], a['ldg'], a['n_cols'], a['c'], a['xp'], a['xi'],
                                    a['prefix'], a['pbits'], a['dbits'], a['hist'], a['splits'], a['ws'], a['ws_bytes'], mem.stream)
    mem.synchronize()
    h = mem.to_host(hist, (bins + PAD,), np.uint64)
    w = mem.to_host(ws, (need + 256,), np.uint8)
    return rc, h[:bins].copy(), bool((h[bins:] == SENT).all() and (w[need:] == 0x5A).all())


def raw_digits(raw, prefix, prefix_bits, digit_bits, ex=None, col_splits=0, start=None, xlists=None):
    if xlists is None and ex is not None:
        xlists = lists_of(ex)
    rc, h, intact = call_digits(raw, prefix, prefix_bits, digit_bits, xlists, col_splits, start)
    raw.rt.check(rc)
    assert intact, 'memory behind the histogram or behind the workspace changed'
    return h


def digits_case(dtype, m, n_cols, ranks, signed=False, pattern='edges', splits=SPLITS, n=None):
    """Every pass of the selection of the n-th candidate: the histogram is np.bincount of the host's keys under the same prefix
    (rows >= m and columns >= n_cols, excluded pairs and NaN scores are in no bin), for every col_splits; a second call on
    the result doubles the counts."""
    G_row, S, G_col = (signed_lattice_factors if signed else lattice_factors)(m, n_cols, ranks)
    H = np.dot(G_row, S)
    H[m // 2, 0] = np.nan                                            # a row of NaN scores: in no bin
    X = np.dot(H, G_col.T)
    raw = Raw(dtype, H, G_col)
    ex = exclusion_mask(pattern, m, n_cols)
    order = host_order(X, ex)
    keys = host_keys(order[2], NPT[dtype])
    assert keys.size == (~np.isnan(X) & (True if ex is None else ~ex)).sum() and (np.diff(keys.astype(object)) <= 0).all()
    n = keys.size // 3 if n is None else n
    bits = 8 * np.dtype(NPT[dtype]).itemsize
    prefix, pbits, left = 0, 0, n
    for db in PLAN[dtype]:
        under = keys[(keys >> np.uint64(bits - pbits)) == prefix] if pbits else keys
        want = np.bincount(((under >> np.uint64(bits - pbits - db)) & np.uint64((1 << db) - 1)).astype(np.int64), minlength=1 << db)
        what = 'digits %s m %d n_cols %d ranks %r prefix %d/%d' % (dtype, m, n_cols, ranks, prefix, pbits)
        for s in splits:
            got = raw_digits(raw, prefix, pbits, db, ex, col_splits=s)
            assert np.array_equal(got, want.astype(np.uint64)), '%s splits %d: the histogram differs from the host keys' % (what, s)
        twice = raw_digits(raw, prefix, pbits, db, ex, start=got)
        assert np.array_equal(twice, 2 * want.astype(np.uint64)), what + ': a second call does not add to the histogram'
        d, above = digit_walk(want, left)
        left -= above
        prefix, pbits = (prefix << db) | d, pbits + db
    assert prefix == int(keys[n - 1]), 'the walk over the host histograms does not end at the n-th key'
    # no row: success, nothing added
    start = np.arange(2048, dtype=np.uint64)
    assert np.array_equal(raw_digits(Raw(dtype, H[:0], G_col), 0, 0, 11, start=start), start)
    assert np.array_equal(raw_digits(Raw(dtype, H, G_col[:0]), 0, 0, 11, start=start), start)


def digit_walk_case(seed=0):
    """digit_walk is a pure function of the histograms: against a sort of random 32-bit keys with heavy ties."""
    rs = np.random.RandomState(seed)
    keys = rs.randint(0, 2 ** 32, size=40, dtype=np.uint64)[rs.randint(0, 40, size=5000)]
    keys[:7] = 0xFFFFFFFF
    srt = np.sort(keys)[::-1]
    for n in (1, 7, 8, 2500, 5000, 5007):
        prefix, pbits, left, greater = 0, 0, min(n, keys.size), 0
        for db in (11, 11, 10):
            under = keys[(keys >> np.uint64(32 - pbits)) == prefix] if pbits else keys
            counts = np.bincount(((under >> np.uint64(32 - pbits - db)) & np.uint64((1 << db) - 1)).astype(np.int64), minlength=1 << db)
            d, above = digit_walk(counts, left)
            left, greater = left - above, greater + above
            prefix, pbits = (prefix << db) | d, pbits + db
        kth = int(srt[min(n, keys.size) - 1])
        assert prefix == kth and greater == int((keys > kth).sum()) and 1 <= left <= int((keys == kth).sum()), n
    assert digit_walk(np.zeros(2048, dtype=np.uint64), 3) == (None, 0)
    assert digit_walk(np.array([0, 2, 0, 3, 0], dtype=np.uint64), 9) == (1, 3)       # too few: the lowest bin that holds one
    assert digit_walk(np.array([2 ** 63, 2 ** 63, 5], dtype=np.uint64), 2 ** 63 + 6) == (0, 2 ** 63 + 5)   # no 64-bit wrap


def refusals_without_device(lib, ptr):
    """Everything refused before any HIP call (`ptr`: any non-null, 256-byte aligned address; it is never dereferenced)."""
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    need = C.c_size_t()
    assert lib.skf_complete_digits_workspace_bytes(nat.SKF_F32, 67, 203, 0, C.byref(need)) == 0
    nb = need.value
    assert 256 <= nb < 4096, 'flag words: nothing of the size of the relation'

    def digits(dtype=nat.SKF_F32, H=ptr, Gc=ptr, c=8, ldh=8, ldg=8, xp=None, xi=None, prefix=0, pbits=0, dbits=11, hist=ptr, ws=ptr,
               ws_bytes=nb, splits=0, m=67, n_cols=203):
        return lib.skf_complete_digits(dtype, H, ldh, m, Gc, ldg, n_cols, c, xp, xi, prefix, pbits, dbits, hist, splits, ws, ws_bytes, None)
    for kw in (dict(dtype=nat.SKF_BF16), dict(dtype=7), dict(m=-1), dict(m=2 ** 31), dict(n_cols=-1), dict(n_cols=2 ** 31), dict(c=0),
               dict(c=1025), dict(H=None), dict(Gc=None), dict(hist=None), dict(ldh=7), dict(ldg=7), dict(splits=-1), dict(splits=33),
               dict(xp=ptr), dict(xi=ptr), dict(dbits=0), dict(dbits=12), dict(dbits=-1), dict(pbits=-1), dict(pbits=22, dbits=11),
               dict(pbits=32, dbits=1), dict(dtype=nat.SKF_F64, pbits=54, dbits=11), dict(pbits=11, prefix=2048), dict(prefix=1),
               dict(dtype=nat.SKF_F64, pbits=63, dbits=1, prefix=2 ** 63)):
        assert digits(**kw) == INV, kw
        assert b'skf_complete_digits' in lib.skf_last_error(), kw
    assert digits(ws_bytes=nb - 1) == WS and digits(ws=None) == WS and digits(ws=ptr + 8) == WS
    for kw in (dict(splits=33), dict(splits=-1), dict(m=-1), dict(m=2 ** 31), dict(n_cols=2 ** 31), dict(dtype=nat.SKF_BF16)):
        assert lib.skf_complete_digits_workspace_bytes(kw.get('dtype', nat.SKF_F32), kw.get('m', 67), kw.get('n_cols', 203),
                                                       kw.get('splits', 0), C.byref(need)) == INV, kw
    assert lib.skf_complete_digits_workspace_bytes(nat.SKF_F32, 67, 203, 0, None) == INV
    assert lib.skf_complete_digits_workspace_bytes(nat.SKF_F64, 2 ** 31 - 1, 2 ** 31 - 1, 32, C.byref(need)) == 0 and need.value == nb


def refusals_case(dtype='f64'):
    """Every refusal leaves the histogram as it was, the invalid exclusion lists included."""
    from ranks_cases import defective_lists
    rt = nat.get_runtime()
    keep = rt.mem.empty(16384)
    refusals_without_device(rt.lib, keep.ptr)
    m, n_cols = 37, 70
    G_row, S, G_col = lattice_factors(m, n_cols, (5, 7))
    H = np.dot(G_row, S)
    raw = Raw(dtype, H, G_col)
    ex = exclusion_mask('edges', m, n_cols)
    xl = lists_of(ex)
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    bits = raw.T(0).nbytes * 8
    start = np.arange(2048, dtype=np.uint64) * np.uint64(3)
    nb = digits_workspace(raw)
    for want, over in ((INV, dict(dtype=nat.SKF_BF16)), (INV, dict(m=-1)), (INV, dict(m=2 ** 31)), (INV, dict(n_cols=-1)),
                       (INV, dict(n_cols=2 ** 31)), (INV, dict(c=0)), (INV, dict(c=1025)), (INV, dict(H=None)), (INV, dict(Gc=None)),
                       (INV, dict(ldh=raw.c - 1)), (INV, dict(ldg=raw.c - 1)), (INV, dict(splits=-1)), (INV, dict(splits=33)),
                       (INV, dict(xp=None)), (INV, dict(xi=None)), (INV, dict(dbits=0)), (INV, dict(dbits=12)), (INV, dict(pbits=-1)),
                       (INV, dict(pbits=bits - 10)), (INV, dict(pbits=11, prefix=2048)), (INV, dict(prefix=1)),
                       (WS, dict(ws_bytes=nb - 1)), (WS, dict(ws=None))):
        rc, h, intact = call_digits(raw, 0, 0, 11, xl, start=start, **over)
        assert rc == want and b'skf_complete_digits' in rt.lib.skf_last_error(), over
        assert np.array_equal(h, start) and intact, '%r: the histogram was written' % (over,)
    rc, h, intact = call_digits(raw, 0, 0, 11, xl, start=start, hist=None)
    assert rc == INV
    ws = rt.mem.empty(nb + 256)
    rc, h, intact = call_digits(raw, 0, 0, 11, xl, start=start, ws=ws.ptr + 8, ws_bytes=nb)
    assert rc == WS and b'aligned' in rt.lib.skf_last_error() and np.array_equal(h, start)
    for name, (p, i, n) in defective_lists(xl[0], xl[1], m, n_cols).items():
        if name in ('count does not match indptr[m]', 'indptr does not end at its count'):
            continue                                             # (the exclusion lists carry no count but indptr[m])
        for s in (1, 2):
            rc, h, intact = call_digits(raw, 0, 0, 11, (p, i), col_splits=s, start=start)
            assert rc == INV and b'exclusion lists' in rt.lib.skf_last_error(), 'exclusion: ' + name
            assert np.array_equal(h, start) and intact, 'exclusion: %s: the histogram was written' % name
    h = raw_digits(raw, 0, 0, 11, ex, start=start)                   # the lists as they were are accepted
    assert int((h - start).sum()) == int((~ex).sum())


def refusal_order_case(which, dtype='f64'):
    """4 rows x 6 columns with defective exclusion lists: refused by the validation kernel alone."""
    import known_csr_cases as KC
    G_row, S, G_col = lattice_factors(4, 6, (2, 2))
    raw = Raw(dtype, np.dot(G_row, S), G_col)
    KC.refused_after_one_launch(lambda w: raw_digits(raw, 0, 0, 11, xlists=KC.small_lists(w)), which)


# ---- 3. P3 and agreement ---------------------------------------------------------------------------------------------------
def agreement_case(dtype, m, n_cols, ranks, pattern='edges', factors=lattice_factors, ns=(1, 64, 1000)):
    G_row, S, G_col = factors(m, n_cols, ranks)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    fit, rel = model(G_row, S, G_col)
    ex = exclusion_mask(pattern, m, n_cols)
    xl = None if ex is None else lists_of(ex)
    xs = None if ex is None else sparse_of(ex)
    what = 'best agreement %s m %d n_cols %d ranks %r %s' % (dtype, m, n_cols, ranks, pattern)
    tied = 0
    for n in ns:
        T, g, e, cands = comp.kth(blocks_of(G_row, xl, 8192), n)
        assert g < min(n, cands) <= g + e, '%s n %d: %d above, %d equal' % (what, n, g, e)
        for s, step in ((0, 8192), (3, 64), (32, 100)):               # P3: for every col_splits and every cut into blocks
            vals = np.concatenate([comp.above(A, T, exclude=x, col_splits=s)[2] for A, x in blocks_of(G_row, xl, step)()])
            assert vals.size == g + e and int((vals > T).sum()) == g and int((vals == T).sum()) == e, \
                '%s n %d: above(T) holds %d entries, %d above T; kth said %d + %d' % (what, n, vals.size, (vals > T).sum(), g, e)
        tied += e > 1
        # returned pairs against the rank pass: the rank within the row is smaller than the row's entry count
        best = fit.complete_best(rel, n, exclude=xs, dtype=dtype)
        assert best.nnz == min(n, cands)
        pick = np.unique(np.linspace(0, best.nnz - 1, 40).astype(np.int64))
        rows = np.repeat(np.arange(m), np.diff(best.indptr))[pick]
        rank = fit.complete_ranks(rel, rows, best.indices[pick], exclude=xs, dtype=dtype)
        per_row = np.diff(best.indptr)[rows]
        assert ((rank >= 0) & (rank < per_row)).all(), '%s n %d: a returned pair ranks behind its row\'s entry count' % (what, n)
    return tied


def single_row_case(dtype, n_cols, ranks, pattern='edges', factors=lattice_factors):
    """m = 1 and n <= 64: complete_best is complete_topk's list, index for index and bit for bit."""
    G_row, S, G_col = factors(3, n_cols, ranks)
    fit, rel = model(G_row, S, G_col)
    ex = exclusion_mask(pattern, 3, n_cols)
    xs = None if ex is None else sparse_of(ex)
    for n in (1, 8, 64):
        ti, tv = fit.complete_topk(rel, n, rows=[2], exclude=xs, dtype=dtype)
        have = int((ti[0] >= 0).sum())
        best = fit.complete_best(rel, n, rows=[2], exclude=xs, dtype=dtype)
        assert best.shape == (1, n_cols) and best.nnz == have == min(n, n_cols if ex is None else int((~ex[2]).sum()))
        o = np.argsort(-best.data, kind='stable')
        assert np.array_equal(best.indices[o], ti[0, :have]), 'single row %s n %d: not top-k\'s columns' % (dtype, n)
        assert best.data[o].tobytes() == tv[0, :have].tobytes(), 'single row %s n %d: not top-k\'s bits' % (dtype, n)


# ---- 4. random cases -------------------------------------------------------------------------------------------------------
def check_random(got, T, n, X64, B, ex, what):
    """The random-case conditions on a result of complete_best (CSR over the rows of X64) with the device's threshold T."""
    m, ncol = X64.shape
    ok = np.ones((m, ncol), dtype=bool) if ex is None else ~ex
    sel = np.zeros((m, ncol), dtype=bool)
    r_of = np.repeat(np.arange(m), np.diff(got.indptr))
    sel[r_of, got.indices] = True
    Bm = float(B.max())
    band = int((ok & (np.abs(X64 - T) <= 2 * Bm)).sum())
    ratio = float((np.abs(got.data - X64[r_of, got.indices]) / B[r_of, got.indices]).max())
    line = '%s: %d entries, threshold %.9g, max |value - X64| / b = %.3g, %d of %d admissible pairs in the band' % (
        what, got.nnz, T, ratio, band, ok.sum())
    print(line)
    DEVIATIONS.append(line)
    assert got.nnz == n == sel.sum(), '%s: %d entries, %d wanted' % (what, got.nnz, n)
    assert not (sel & ~ok).any(), what + ': an excluded pair was selected'
    assert got.data.min() == T, what + ': the smallest value is not the threshold'
    assert ratio <= 1.0, '%s: a value is %.3e x its bound away' % (what, ratio)
    missing = ok & (X64 > T + Bm) & ~sel
    assert not missing.any(), '%s: %d pairs more than B above the threshold are absent' % (what, missing.sum())
    wrong = sel & (X64 < T - Bm)
    assert not wrong.any(), '%s: %d pairs more than B below the threshold are present' % (what, wrong.sum())
    assert band <= 0.001 * ok.sum(), '%s: %d of %d pairs are undecided: the test decides too little' % (what, band, ok.sum())
    return band


def random_case(dtype, ranks, m=131, n_cols=997, n=2000, pattern='heavy', label=''):
    T_ = NPT[dtype]
    G_row, S, G_col = (x.astype(T_).astype(np.float64) for x in random_factors(m, n_cols, ranks))   # rounded to the scoring type
    X64 = np.dot(np.dot(G_row, S), G_col.T)
    B = bound(G_row, S, G_col, dtype)
    ex = exclusion_mask(pattern, m, n_cols)
    fit, rel = model(G_row, S, G_col)
    xs = None if ex is None else sparse_of(ex)
    what = '%s best random %s %dx%d ranks %r %s n %d' % (label, dtype, m, n_cols, ranks, pattern, n)
    T, g, e = fit.complete_kth(rel, n, exclude=xs, dtype=dtype)
    assert g < n <= g + e
    got = fit.complete_best(rel, n, exclude=xs, dtype=dtype)
    check_random(got, T, n, X64, B, ex, what)
    return got


# ---- 5. NaN and infinities ---------------------------------------------------------------------------------------------------
def nan_inf_case(dtype, m=67, n_cols=203, ranks=(5, 2)):
    G_row, S, G_col = lattice_factors(m, n_cols, ranks)
    S[0] = np.maximum(S[0], 0.125)
    G_row[9, 1] = np.nan                                             # a NaN row: never selected, never counted
    G_row[4] = 0.0
    G_row[4, 0] = np.inf                                             # row 4: +inf in the columns whose factor row has no zero,
    G_row[11] = 0.0                                                  # NaN (inf * 0) in the others
    G_row[11, 0] = -np.inf                                           # row 11: -inf / NaN
    with np.errstate(invalid='ignore'):
        X = np.dot(np.dot(G_row, S), G_col.T)
    assert np.isnan(X[9]).all() and np.isposinf(X[4]).sum() > 70 and np.isneginf(X[11]).sum() > 70
    ex = exclusion_mask('edges', m, n_cols)
    order = host_order(X, ex)
    cands, n_pos = order[2].size, int(np.isposinf(order[2]).sum())
    assert cands == int((~np.isnan(X) & ~ex).sum()) and cands < int((~ex).sum()) - n_cols // 2
    fit, rel = model(G_row, S, G_col)
    xs = sparse_of(ex)
    what = 'best NaN / inf %s' % dtype
    # +inf first, with more tied pairs than wanted (the strict threshold above +inf is NaN); the whole tie; one past it;
    # everything, -inf last; more than everything
    for n in (1, n_pos // 2, n_pos, n_pos + 1, cands - 3, cands, cands + 9):
        want = host_kth(order, n)
        same_kth(fit.complete_kth(rel, n, exclude=xs, dtype=dtype) + (cands,), want, '%s n %d' % (what, n))
        for ties in ('first', 'all'):
            for step in (8192, 3):
                got = fit.complete_best(rel, n, exclude=xs, dtype=dtype, ties=ties, block_rows=step)
                same_csr(got, host_best(order, n, X.shape, ties), '%s n %d ties %s block_rows %d' % (what, n, ties, step))
                assert got[9].nnz == 0 and not np.isnan(got.data).any()
    assert host_kth(order, n_pos // 2)[0] == np.inf and host_kth(order, cands)[0] == -np.inf
    # no candidate at all: T is NaN, the result empty
    T, g, e = fit.complete_kth(rel, 5, rows=[9, 9], dtype=dtype)
    assert np.isnan(T) and (g, e) == (0, 0)
    got = fit.complete_best(rel, 5, rows=[9, 9], dtype=dtype)
    assert got.shape == (2, n_cols) and got.nnz == 0


# ---- 6. independence -----------------------------------------------------------------------------------------------------------
def independence_case(dtype, m=131, n_cols=203, ranks=(20, 64), n=700, pattern='edges'):
    G_row, S, G_col = random_factors(m, n_cols, ranks)
    G_row = np.round(G_row * 16) / 16                                # a coarse row factor: ties survive the random columns
    ex = exclusion_mask(pattern, m, n_cols)
    xl = lists_of(ex)
    fit, rel = model(G_row, S, G_col)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    first = comp.kth(blocks_of(G_row, xl, 8192), n)
    for step in (64, 100, 8192):
        for s in SPLITS:
            got = comp.kth(blocks_of(G_row, xl, step), n, col_splits=s)
            assert got == first, 'kth %s block_rows %d col_splits %d: %r, before %r' % (dtype, step, s, got, first)
    out = [csr_bytes(fit.complete_best(rel, n, exclude=sparse_of(ex), dtype=dtype, block_rows=step, ties=ties))
           for ties in ('first', 'all') for step in (64, 100, 8192)]
    assert out[0] == out[1] == out[2] and out[3] == out[4] == out[5], 'complete_best %s: block_rows changes the bytes' % dtype
    return out[0]


# ---- 7. public API ----------------------------------------------------------------------------------------------------------
def api_case(kind, monkeypatch):
    """The fitted models of above_cases.api_case ('dfmc-masked' with exclude='known', 'dfmf-csr'); the comparison with
    complete() runs in f64 on a model whose factors were rounded to a coarse lattice, so that the host order is exact."""
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
    known = ~np.ma.getmaskarray(data) if np.ma.isMaskedArray(data) else _pattern(data)
    what = 'api best %s' % kind

    def boom(*a, **kw):
        raise AssertionError('the dense reconstruction was formed')
    monkeypatch.setattr(FusionFit, 'complete', boom)
    monkeypatch.setattr(FusionFit, '_reconstruct', boom)
    for exclude, ex in ((None, None), ('known', known)):
        order = host_order(X, ex)
        for n in (1, 37, 400):
            same_kth(fuser.complete_kth(rel, n, exclude=exclude) + (order[2].size,), host_kth(order, n), '%s kth n %d' % (what, n))
            for ties in ('first', 'all'):
                same_csr(fuser.complete_best(rel, n, exclude=exclude, ties=ties, block_rows=7), host_best(order, n, X.shape, ties),
                         '%s n %d ties %s' % (what, n, ties))
    # rows in arbitrary order with a duplicate: a row listed twice is two rows, the earlier position wins the tie
    rows = np.array([17, 3, 3, 39, 0])
    order = host_order(X[rows], known[rows])
    for n in (1, 10, 60, order[2].size + 1):
        got = fuser.complete_best(rel, n, rows=rows, exclude='known', block_rows=2)
        same_csr(got, host_best(order, n, (5, n_j), 'first'), '%s rows= n %d' % (what, n))
        assert fuser.complete_kth(rel, n, rows=rows, exclude='known', block_rows=2) == host_kth(order, n)[:3]
    two = fuser.complete_best(rel, 2 * n_j, rows=[3, 3])
    assert two.shape == (2, n_j) and two.nnz == 2 * n_j and csr_bytes(two[0]) == csr_bytes(two[1])
    # n = 0, no rows, the result as the next exclusion
    assert fuser.complete_best(rel, 0).nnz == 0 and fuser.complete_best(rel, 0).shape == (n_i, n_j)
    T, g, e = fuser.complete_kth(rel, 0)
    assert np.isnan(T) and (g, e) == (0, 0)
    assert fuser.complete_best(rel, 5, rows=np.zeros(0, dtype=int)).shape == (0, n_j)
    top = fuser.complete_best(rel, 100)
    nxt = fuser.complete_best(rel, 100, exclude=top)
    assert nxt.nnz == 100 and top.multiply(nxt).nnz == 0 and nxt.data.max() <= top.data.min()
    # 'bf16' scores on the f32 masters
    a, b = fuser.complete_best(rel, 50, exclude='known', dtype='f32'), fuser.complete_best(rel, 50, exclude='known', dtype='bf16')
    assert csr_bytes(a) == csr_bytes(b) and a.nnz == 50
    assert fuser.complete_kth(rel, 50, exclude='known', dtype='f32') == fuser.complete_kth(rel, 50, exclude='known', dtype='bf16')
    # refusals
    with pytest.raises(DataFusionError, match='negative'):
        fuser.complete_best(rel, -1)
    with pytest.raises(DataFusionError, match='negative'):
        fuser.complete_kth(rel, -1)
    with pytest.raises(DataFusionError, match='max_entries'):
        fuser.complete_best(rel, 11, max_entries=10)
    assert fuser.complete_best(rel, 10, max_entries=10).nnz == 10
    with pytest.raises(DataFusionError, match='ties'):
        fuser.complete_best(rel, 10, ties='last')
    with pytest.raises(DataFusionError):
        fuser.complete_best(rel, 10, rows=[n_i])
    with pytest.raises(DataFusionError, match='shape'):
        fuser.complete_best(rel, 10, exclude=scipy.sparse.csr_matrix((n_i, n_j - 1)))
    post = Relation(rel.data, users, movies, postprocessor=lambda x: np.clip(x, 0.0, 1.0),
                    **({'unstored': rel.unstored} if scipy.sparse.issparse(rel.data) else {}))
    fuser.backbones_[post] = fuser.backbones_[rel]
    for method in (fuser.complete_best, fuser.complete_kth):
        with pytest.raises(DataFusionError, match='postprocessor'):
            method(post, 10)


def _pattern(data):
    """Boolean [n_i, n_j] of the stored entries of a scipy.sparse matrix, without expanding it through scipy."""
    coo = data.tocoo()
    out = np.zeros(data.shape, dtype=bool)
    out[coo.row, coo.col] = True
    return out


def api_runs_case():
    """n_run = 2 and run=None: a generator over the runs, each equal to the explicit run."""
    import types
    import known_csr_api_cases as KA
    from skfusion_amd.fusion import Dfmc
    _, ma = KA.ratings(40, 30, 0.2, 11)
    g, users, movies = KA.graph(ma, ranks=(5, 4, 3))
    fuser = KA.fit(Dfmc, g, max_iter=3, init_type='random', random_state=0, dtype='f64', n_run=2)
    rel = list(g.relations)[0]
    out, kth = fuser.complete_best(rel, 25, exclude='known'), fuser.complete_kth(rel, 25, exclude='known')
    assert isinstance(out, types.GeneratorType) and isinstance(kth, types.GeneratorType)
    out, kth = list(out), list(kth)
    assert len(out) == len(kth) == 2
    for r in range(2):
        assert csr_bytes(out[r]) == csr_bytes(fuser.complete_best(rel, 25, exclude='known', run=r)) and out[r].nnz == 25
        assert kth[r] == fuser.complete_kth(rel, 25, exclude='known', run=r) and out[r].data.min() == kth[r][0]
    assert csr_bytes(out[0]) != csr_bytes(out[1])
