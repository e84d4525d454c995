"""Top-k completion and entry predictions without the dense reconstruction (csrc/skf_complete.h, skf_complete_topk /
skf_complete_entries, _engine.DeviceCompleter, FusionFit.complete_topk / complete_entries) -- the SAME cases on the host
emulator (small) and on the GPU.  The yardstick is always host NumPy in float64.

  1. exact cases: G_row, S, G_col hold multiples of 1/8 in [0, 7/8].  With ranks <= 128 every H = G_row S entry is a multiple
     of 1/64 below 2^13 / 64 and every score a multiple of 1/512 with a numerator below 128 * 128 * 7^3 < 2^23: every partial
     sum is exact in f32 whatever the order, so the device must give the float64 result bit for bit and the host's order --
     stable argsort by (-score, index) -- index for index.  At rank 5 fewer than a fifth of the scores of a row are distinct.
  2. random cases: with u = 2^-24 / 2^-53 and n = c_i + c_j + 5, b(r, j) = n u / (1 - n u) (|G_row| |S| |G_col|^T)[r, j] is
     the standard forward bound of the two chained dot products plus the roundings of the inputs to the engine's type, valid
     for every summation order.  Every row must hold distinct, admissible columns in the total order, values within b of
     X64, and no other admissible column may beat the worst selected one by more than 2 max_j b(r, j).
  3. refusals: every SKF_E_INVALID / SKF_E_WORKSPACE of the header comment, outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DeviceCompleter
from helpers import within

NPT = {'f64': np.float64, 'f32': np.float32, 'bf16': np.float32}
UNIT = {'f64': 2.0 ** -53, 'f32': 2.0 ** -24, 'bf16': 2.0 ** -24}
WORST = {}                     # dtype -> largest |out_val - X64| / b seen (reported by the GPU module)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def lattice(rs, shape):
    return rs.randint(0, 8, size=shape) / 8.0


def lattice_factors(m, n_cols, ranks, seed=0):
    rs = np.random.RandomState(seed + 1000 * ranks[0] + ranks[1])
    return lattice(rs, (m, ranks[0])), lattice(rs, (ranks[0], ranks[1])), lattice(rs, (n_cols, ranks[1]))


def random_factors(m, n_cols, ranks, seed=0):
    rs = np.random.RandomState(seed + ranks[0])
    return rs.rand(m, ranks[0]) * 0.1 + 0.01, rs.rand(ranks[0], ranks[1]) * 0.2, rs.rand(n_cols, ranks[1]) * 0.1 + 0.01


def exclusion_mask(pattern, m, n_cols, seed=0):
    """Boolean [m, n_cols] of the excluded pairs, or None ('none'); 'empty': lists are given and hold nothing."""
    if pattern == 'none':
        return None
    ex = np.zeros((m, n_cols), dtype=bool)
    if pattern == 'empty':
        return ex
    rs = np.random.RandomState(seed + 7)
    ex |= rs.rand(m, n_cols) < 0.125
    if pattern == 'edges':
        for j in (0, 63, 64, n_cols - 1):
            if 0 <= j < n_cols:
                ex[:, j] = True
    elif pattern == 'heavy':
        ex[3 % m, :] = True                                     # no candidate at all
        ex[(m - 2) % m, :] = True                               # three candidates
        ex[(m - 2) % m, rs.choice(n_cols, size=min(3, n_cols), replace=False)] = False
    else:
        raise ValueError(pattern)
    return ex


def lists_of(ex):
    indptr = np.zeros(ex.shape[0] + 1, dtype=np.int64)
    np.cumsum(ex.sum(axis=1), out=indptr[1:])
    return indptr, np.nonzero(ex)[1].astype(np.int32)


# ---- the host's answer -------------------------------------------------------------------------------------------------------
def host_topk(X, k, ex=None):
    """Stable argsort by (-score, index) over the admissible columns; padding -1 / -inf."""
    m, n = X.shape
    idx = np.full((m, k), -1, dtype=np.int32)
    val = np.full((m, k), -np.inf)
    for r in range(m):
        ok = ~np.isnan(X[r])
        if ex is not None:
            ok &= ~ex[r]
        cand = np.nonzero(ok)[0]
        order = cand[np.argsort(-X[r, cand], kind='stable')][:k]
        idx[r, :order.size] = order
        val[r, :order.size] = X[r, order]
    return idx, val


def bound(G_row, S, G_col, dtype):
    n = S.shape[0] + S.shape[1] + 5
    g = n * UNIT[dtype] / (1.0 - n * UNIT[dtype])
    return g * np.dot(np.abs(G_row), np.dot(np.abs(S), np.abs(G_col).T))


def check_conditions(idx, val, X64, B, ex, k, what):
    """The random-case conditions, every row, no exemption.  Returns the largest |val - X64| / b."""
    m, n = X64.shape
    worst = 0.0
    assert idx.shape == (m, k) and val.shape == (m, k) and idx.dtype == np.int32, what
    for r in range(m):
        ok = np.ones(n, dtype=bool) if ex is None else ~ex[r]
        have = min(k, int(ok.sum()))
        sel = idx[r, :have].astype(np.int64)
        assert (idx[r, have:] == -1).all() and np.isneginf(val[r, have:]).all(), '%s row %d: padding' % (what, r)
        assert ((sel >= 0) & (sel < n)).all() and np.unique(sel).size == have, '%s row %d: indices not distinct / in range' % (what, r)
        assert ok[sel].all(), '%s row %d: an excluded column was selected' % (what, r)
        v = val[r, :have]
        step_ok = (v[:-1] > v[1:]) | ((v[:-1] == v[1:]) & (sel[:-1] < sel[1:]))
        assert step_ok.all(), '%s row %d: not in the total order' % (what, r)
        if have == 0:
            continue
        ratio = np.abs(v - X64[r, sel]) / B[r, sel]
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), '%s row %d: value %.3e x its bound' % (what, r, ratio.max())
        rest = ok.copy()
        rest[sel] = False
        if rest.any():
            over = X64[r, rest].max() - (X64[r, sel].min() + 2.0 * B[r].max())
            assert over <= 0.0, '%s row %d: a better column was left out by %.3e' % (what, r, over)
    return worst


# ---- the C ABI, called directly ----------------------------------------------------------------------------------------------
class Raw(object):
    """skf_complete_topk / skf_complete_entries on host-made H with padded leading dimensions and sentinels behind them."""

    def __init__(self, dtype, H, Gc):
        self.rt = nat.get_runtime()
        self.code, self.T = nat.DTYPES[dtype], NPT[dtype]
        self.m, self.c = H.shape
        self.n_cols = Gc.shape[0]
        self.ldh, self.ldg = self.c + 3, self.c + 1
        Hp = np.full((max(self.m, 1), self.ldh), 99.0, dtype=self.T)
        Gp = np.full((max(self.n_cols, 1), self.ldg), -99.0, dtype=self.T)
        Hp[:self.m, :self.c] = H
        Gp[:self.n_cols, :self.c] = Gc
        self.h, self.g = self.rt.mem.from_host(Hp), self.rt.mem.from_host(Gp)

    def workspace(self, k, col_splits, m=None):
        need = C.c_size_t()
        self.rt.call('skf_complete_topk_workspace_bytes', self.code, self.m if m is None else m, self.n_cols, k, col_splits, C.byref(need))
        return need.value

    def topk(self, k, ex=None, col_splits=0, lists=None, status=False):
        rt, mem = self.rt, self.rt.mem
        ldi, ldv = k + 2, k + 1
        oi = mem.from_host(np.full((self.m, ldi), -7, dtype=np.int32))
        ov = mem.from_host(np.full((self.m, ldv), -7.0, dtype=self.T))
        ws = mem.empty(self.workspace(k, col_splits))
        xp = xi = None
        if lists is None and ex is not None:
            lists = lists_of(ex)
        if lists is not None:
            xp = mem.from_host(np.asarray(lists[0], dtype=np.int64))
            xi = mem.from_host(np.asarray(lists[1], dtype=np.int32) if len(lists[1]) else np.zeros(1, dtype=np.int32))
        rc = rt.lib.skf_complete_topk(self.code, self.h.ptr, self.ldh, self.m, self.g.ptr, self.ldg, self.n_cols, self.c, k,
                                      xp.ptr if xp else None, xi.ptr if xi else None, oi.ptr, ldi, ov.ptr, ldv, col_splits,
                                      ws.ptr, ws.nbytes, mem.stream)
        mem.synchronize()
        gi, gv = mem.to_host(oi, (self.m, ldi), np.int32), mem.to_host(ov, (self.m, ldv), self.T)
        if status:
            return rc, gi, gv
        rt.check(rc)
        assert (gi[:, k:] == -7).all() and (gv[:, k:] == -7.0).all(), 'memory behind slot k changed'
        return gi[:, :k].copy(), gv[:, :k].copy()

    def entries(self, rows, cols, status=False):
        rt, mem = self.rt, self.rt.mem
        n = len(rows)
        o = mem.from_host(np.full(n + 1, -7.0, dtype=self.T))
        br, bc = mem.from_host(np.asarray(rows, dtype=np.int32)), mem.from_host(np.asarray(cols, dtype=np.int32))
        rc = rt.lib.skf_complete_entries(self.code, self.h.ptr, self.ldh, self.m, self.g.ptr, self.ldg, self.n_cols, self.c,
                                         br.ptr, bc.ptr, n, o.ptr, mem.stream)
        mem.synchronize()
        out = mem.to_host(o, (n + 1,), self.T)
        if status:
            return rc, out
        rt.check(rc)
        assert out[n] == -7.0, 'memory behind entry n changed'
        return out[:n].copy()


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------
def exact_case(dtype, m, n_cols, ranks, ks=(1, 10, 64), patterns=('none', 'empty', 'edges', 'heavy'), splits=(0, 1, 2, 3)):
    G_row, S, G_col = lattice_factors(m, n_cols, ranks)
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    assert X.max() * 512 < 2 ** 23 and np.array_equal(X.astype(np.float32).astype(np.float64), X)      # exact in f32
    raw = Raw(dtype, H, G_col)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    for pattern in patterns:
        ex = exclusion_mask(pattern, m, n_cols)
        for k in ks:
            what = 'topk exact %s m %d n %d ranks %r k %d %s' % (dtype, m, n_cols, ranks, k, pattern)
            hi, hv = host_topk(X, k, ex)
            first = None
            for s in splits:
                gi, gv = raw.topk(k, ex, col_splits=s)
                assert np.array_equal(gi, hi), '%s splits %d: indices differ from the host order' % (what, s)
                assert np.array_equal(gv.astype(np.float64), hv), '%s splits %d: values differ from the host scores' % (what, s)
                if first is None:
                    first = (gi.tobytes(), gv.tobytes())
                assert (gi.tobytes(), gv.tobytes()) == first, '%s: col_splits %d changes the bytes' % (what, s)
            if k > n_cols or pattern == 'heavy':
                assert (hi == -1).any()                          # k > candidates: the padding is exercised
        # the engine path (H by skf_gemm) on the last k
        ei, ev = comp.topk(G_row, ks[-1], exclude=None if ex is None else lists_of(ex))
        hi, hv = host_topk(X, ks[-1], ex)
        assert np.array_equal(ei, hi) and np.array_equal(ev, hv), 'DeviceCompleter.topk %s %s' % (dtype, pattern)
    # entries: repeated pairs, the two corners
    rs = np.random.RandomState(3)
    rows = np.concatenate([[0, m - 1, 5 % m, 5 % m], rs.randint(0, m, 300)])
    cols = np.concatenate([[0, n_cols - 1, 2 % n_cols, 2 % n_cols], rs.randint(0, n_cols, 300)])
    assert np.array_equal(raw.entries(rows, cols).astype(np.float64), X[rows, cols]), 'entries exact %s' % dtype
    assert np.array_equal(comp.entries(G_row, rows, cols), X[rows, cols]), 'DeviceCompleter.entries exact %s' % dtype


# ---- 2. random cases -------------------------------------------------------------------------------------------------------
def random_case(dtype, ranks, m=131, n_cols=997, k=10, pattern='edges', label=''):
    G_row, S, G_col = random_factors(m, n_cols, ranks)
    X64 = np.dot(np.dot(G_row, S), G_col.T)
    B = bound(G_row, S, G_col, dtype)
    ex = exclusion_mask(pattern, m, n_cols)
    lists = None if ex is None else lists_of(ex)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    what = '%s topk random %s ranks %r %s' % (label, dtype, ranks, pattern)
    idx, val = comp.topk(G_row, k, exclude=lists)
    worst = check_conditions(idx, val, X64, B, ex, k, what)
    within(worst, 1.0 + 1e-12, what + ': max |val - X64| / b')
    idx2, val2 = comp.topk(G_row, k, exclude=lists)
    assert idx.tobytes() == idx2.tobytes() and val.tobytes() == val2.tobytes(), what + ': two runs differ'
    for s in (1, 3):
        i3, v3 = comp.topk(G_row, k, exclude=lists, col_splits=s)
        assert idx.tobytes() == i3.tobytes() and val.tobytes() == v3.tobytes(), what + ': col_splits %d changes the bytes' % s
    rs = np.random.RandomState(5)
    rows, cols = rs.randint(0, m, 2000), rs.randint(0, n_cols, 2000)
    out = comp.entries(G_row, rows, cols)
    ratio = float((np.abs(out - X64[rows, cols]) / B[rows, cols]).max())
    within(ratio, 1.0 + 1e-12, what + ': entries max |out - X64| / b')
    assert out.tobytes() == comp.entries(G_row, rows, cols).tobytes(), what + ': two runs of entries differ'
    WORST[dtype] = max(WORST.get(dtype, 0.0), worst, ratio)
    return idx, val, out


def bf16_is_f32_case(ranks=(20, 64)):
    a, b = random_case('f32', ranks), random_case('bf16', ranks)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "the 'bf16' engine name must score on the f32 masters"


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------
def refusals_without_device(lib, ptr):
    """Everything refused before any launch (`ptr`: any non-null address; it is never dereferenced)."""
    INV, WS = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE
    need = C.c_size_t()
    assert lib.skf_complete_topk_workspace_bytes(nat.SKF_F32, 67, 203, 10, 0, C.byref(need)) == 0 and need.value >= 256
    nb = need.value

    def topk(dtype=nat.SKF_F32, H=ptr, Gc=ptr, c=8, k=10, xp=None, xi=None, oi=ptr, ov=ptr, ws=ptr, ws_bytes=nb, splits=0, m=67):
        return lib.skf_complete_topk(dtype, H, c, m, Gc, c, 203, c, k, xp, xi, oi, k, ov, k, splits, ws, ws_bytes, None)
    for kw in (dict(k=0), dict(k=65), dict(c=0), dict(c=1025), dict(H=None), dict(Gc=None), dict(oi=None), dict(ov=None),
               dict(xp=ptr), dict(xi=ptr), dict(dtype=nat.SKF_BF16), dict(splits=-1), dict(m=2 ** 31)):
        assert topk(**kw) == INV, kw
        assert b'skf_complete_topk' in lib.skf_last_error()
    assert topk(ws_bytes=nb - 1) == WS and topk(ws=None) == WS
    for s in (1, 2, 3):
        assert lib.skf_complete_topk_workspace_bytes(nat.SKF_F32, 67, 203, 10, s, C.byref(need)) == 0
        assert topk(splits=s, ws_bytes=need.value - 1) == WS, s
    for kw in (dict(k=0), dict(k=65), dict(m=-1)):
        k, m = kw.get('k', 10), kw.get('m', 67)
        assert lib.skf_complete_topk_workspace_bytes(nat.SKF_F32, m, 203, k, 0, C.byref(need)) == INV
    assert lib.skf_complete_topk_workspace_bytes(nat.SKF_F32, 67, 203, 10, 0, None) == INV

    def entries(dtype=nat.SKF_F64, H=ptr, Gc=ptr, c=8, rows=ptr, cols=ptr, out=ptr, n=5):
        return lib.skf_complete_entries(dtype, H, c, 67, Gc, c, 203, c, rows, cols, n, out, None)
    for kw in (dict(c=0), dict(c=1025), dict(H=None), dict(Gc=None), dict(rows=None), dict(cols=None), dict(out=None), dict(n=-1),
               dict(dtype=nat.SKF_BF16)):
        assert entries(**kw) == INV, kw


def refusals_case(dtype='f64'):
    rt = nat.get_runtime()
    keep = rt.mem.empty(4096)
    refusals_without_device(rt.lib, keep.ptr)
    m, n_cols, k = 37, 70, 5
    G_row, S, G_col = lattice_factors(m, n_cols, (5, 7))
    raw = Raw(dtype, np.dot(G_row, S), G_col)
    ex = exclusion_mask('edges', m, n_cols)
    p, i = lists_of(ex)
    a, b = int(p[4]), int(p[5])
    assert b - a >= 2
    bad = {}
    j = i.copy(); j[a], j[a + 1] = i[a + 1], i[a]; bad['descending'] = (p, j)
    j = i.copy(); j[a] = j[a + 1]; bad['repeated'] = (p, j)
    j = i.copy(); j[b - 1] = n_cols; bad['column past the end'] = (p, j)
    j = i.copy(); j[a] = -1; bad['negative column'] = (p, j)
    q = p.copy(); q[0] = 1; bad['indptr does not start at 0'] = (q, i)
    q = p.copy(); q[m] = p[m - 1] - 1; bad['indptr does not end at its count'] = (q, i)
    q = p.copy(); q[m] = -3; bad['negative count'] = (q, i)
    q = p.copy(); q[7] = p[m] + 5; bad['indptr past the count'] = (q, i)
    for name, lists in bad.items():
        for s in (1, 2):
            rc, gi, gv = raw.topk(k, lists=lists, col_splits=s, status=True)
            assert rc == nat.SKF_E_INVALID and b'exclusion lists' in rt.lib.skf_last_error(), name
            assert (gi == -7).all() and (gv == -7.0).all(), name + ': outputs were written'
    gi, gv = raw.topk(k, ex)                                                 # and the lists as they were are accepted
    assert (gi >= -1).all()
    for rows, cols in (([0, m], [0, 0]), ([0, 1], [0, n_cols]), ([-1, 1], [0, 0]), ([0, 1], [3, -1])):
        rc, out = raw.entries(rows, cols, status=True)
        assert rc == nat.SKF_E_INVALID and b'skf_complete_entries' in rt.lib.skf_last_error()
        assert (out == -7.0).all(), 'entries: outputs were written'
    assert raw.entries([m - 1], [n_cols - 1]).shape == (1,)


def refusal_order_case(which, dtype='f64'):
    """Top-k of 4 rows x 6 columns with defective exclusion lists: refused by the validation kernel alone."""
    import known_csr_cases as KC
    G_row, S, G_col = lattice_factors(4, 6, (2, 2))
    raw = Raw(dtype, np.dot(G_row, S), G_col)
    KC.refused_after_one_launch(lambda w: raw.topk(2, lists=KC.small_lists(w)), which)


# ---- 4. public API ------------------------------------------------------------------------------------------------------------
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
    G1, S, G2 = fuser.factor(users), fuser.backbone(rel), fuser.factor(movies)
    B = bound(G1, S, G2, dtype)
    what = 'api %s %s' % (kind, dtype)
    rs = np.random.RandomState(2)
    rows, cols = rs.randint(0, 40, 200), rs.randint(0, 30, 200)
    out = fuser.complete_entries(rel, rows, cols, dtype=dtype)
    assert out.dtype == np.float64 and out.shape == (200,)
    within(float((np.abs(out - X[rows, cols]) / B[rows, cols]).max()), 1.0 + 1e-12, what + ': complete_entries / b')
    idx, val = fuser.complete_topk(rel, 5, exclude='known', dtype=dtype)
    assert not known[np.repeat(np.arange(40), 5)[idx.ravel() >= 0], idx.ravel()[idx.ravel() >= 0]].any(), what + ': a known pair came back'
    within(check_conditions(idx, val, X, B, known, 5, what), 1.0 + 1e-12, what + ': complete_topk / b')
    order = np.array([17, 3, 3, 39, 0])
    i2, v2 = fuser.complete_topk(rel, 5, rows=order, exclude='known', dtype=dtype, block_rows=2)
    assert np.array_equal(i2, idx[order]) and np.array_equal(v2, val[order]), what + ': rows= order'
    pat = scipy.sparse.csr_matrix((np.ones(int(known.sum())), np.nonzero(known)), shape=known.shape)
    for fmt in (pat, pat.tocsc(), pat.tocoo()):
        i3, v3 = fuser.complete_topk(rel, 5, exclude=fmt, dtype=dtype)
        assert np.array_equal(i3, idx) and np.array_equal(v3, val), what + ': exclude= as %s' % fmt.format
    i4, v4 = fuser.complete_topk(rel, 3, dtype=dtype)
    check_conditions(i4, v4, X, B, None, 3, what + ' no exclusion')
    # refusals
    with pytest.raises(DataFusionError, match='shape'):
        fuser.complete_topk(rel, 5, exclude=pat[:, :20], dtype=dtype)
    with pytest.raises(DataFusionError):
        fuser.complete_topk(rel, 0, dtype=dtype)
    with pytest.raises(DataFusionError):
        fuser.complete_topk(rel, 65, dtype=dtype)
    plain = list(g.relations)[1]                                 # movies x genres: a plain ndarray
    with pytest.raises(DataFusionError, match='plain array'):
        fuser.complete_topk(plain, 2, exclude='known', dtype=dtype)
    stranger = Relation(np.zeros((40, 3)), users, ObjectType('strangers', 2))
    with pytest.raises(DataFusionError):
        fuser.complete_topk(stranger, 2, dtype=dtype)
    with pytest.raises(DataFusionError):
        fuser.complete_entries(stranger, [0], [0], dtype=dtype)
    with pytest.raises(DataFusionError):
        fuser.complete_entries(rel, [40], [0], dtype=dtype)
    post = Relation(rel.data, users, movies, postprocessor=lambda x: np.clip(x, 0.0, 1.0), **({} if not sparse else {'unstored': rel.unstored}))
    fuser.backbones_[post] = fuser.backbones_[rel]
    with pytest.raises(DataFusionError, match='postprocessor'):
        fuser.complete_topk(post, 2, dtype=dtype)
    assert np.array_equal(fuser.complete_entries(post, rows, cols, dtype=dtype), np.clip(out, 0.0, 1.0))
    return fuser


def api_runs_case(dtype='f64'):
    """n_run = 2 and run=None: generators over the runs, each equal to the explicit run."""
    import types
    import known_csr_api_cases as KA
    from skfusion_amd.fusion import Dfmc
    _, ma = KA.ratings(40, 30, 0.2, 11)
    g, users, movies = KA.graph(ma, ranks=(5, 4, 3))
    fuser = KA.fit(Dfmc, g, max_iter=3, init_type='random', random_state=0, dtype=dtype, n_run=2)
    rel = list(g.relations)[0]
    tk = fuser.complete_topk(rel, 4, exclude='known', dtype=dtype)
    en = fuser.complete_entries(rel, [0, 5], [1, 2], dtype=dtype)
    assert isinstance(tk, types.GeneratorType) and isinstance(en, types.GeneratorType)
    tk, en = list(tk), list(en)
    assert len(tk) == 2 and len(en) == 2
    for r in range(2):
        i, v = fuser.complete_topk(rel, 4, exclude='known', run=r, dtype=dtype)
        assert np.array_equal(tk[r][0], i) and np.array_equal(tk[r][1], v)
        assert np.array_equal(en[r], fuser.complete_entries(rel, [0, 5], [1, 2], run=r, dtype=dtype))
    assert not np.array_equal(tk[0][1], tk[1][1])
