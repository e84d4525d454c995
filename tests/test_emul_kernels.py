"""Kernel logic on the CPU: the real kernel sources run under the host SIMT emulator
(tests/emul) and are compared with NumPy.  These tests validate indexing / tiling / epilogues
/ the launch schedule; the `-m gpu` tests repeat them on the hardware."""
import ctypes as C

import numpy as np
import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime
from helpers import relerr, within


@pytest.fixture(scope='module')
def rt():
    return emulated_runtime()


class Stored(object):
    """A row-major matrix X inside a larger upload: `off` elements, then the rows of X `X.shape[1] + pad` elements apart
    (the last row without its pad).  Every element of the upload outside X holds `fill` (NaN for floats, 0xFF for bytes):
    .ptr is the device address of X[0, 0], .ld the leading dimension; .download() returns the matrix and asserts that the
    upload around it came back bit for bit."""

    def __init__(self, mem, X, pad=0, off=0, fill=None):
        X = np.ascontiguousarray(X)
        rows, cols = X.shape
        self.mem, self.shape, self.ld, self.off = mem, (rows, cols), cols + pad, off
        if fill is None:
            fill = 0xFF if X.dtype.kind in 'ui' else np.nan
        self.host = np.full(off + (rows - 1) * self.ld + cols, fill, X.dtype)
        self.inside = np.zeros(self.host.shape, bool)
        self._view(self.host)[...] = X
        self._view(self.inside)[...] = True
        self.buf = mem.from_host(self.host)
        self.ptr = self.buf.ptr + off * X.dtype.itemsize

    def _view(self, flat):
        rows, cols = self.shape
        return np.lib.stride_tricks.as_strided(flat[self.off:], (rows, cols), (self.ld * flat.itemsize, flat.itemsize))

    def download(self):
        got = self.mem.to_host(self.buf, self.host.shape, self.host.dtype)
        bits = 'u%d' % got.itemsize
        np.testing.assert_array_equal(got.view(bits)[~self.inside], self.host.view(bits)[~self.inside],
                                      err_msg='elements around the matrix (pad columns, lead-in) changed')
        return self._view(got).copy()


def elementwise(got, want, bound, what):
    """max over the elements of |got - want| / bound, held below 1 (recorded with helpers.within); an element whose bound
    is 0 must be exact."""
    err = np.abs(np.asarray(got).astype(np.longdouble) - want)
    assert np.isfinite(err).all(), '%s: non-finite result' % what
    bound = np.asarray(bound, dtype=np.longdouble)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / bound)
    return within(float(ratio.max()) if ratio.size else 0.0, 1.0, '%s, |got - want| / bound' % what)


def run_gemm(rt, dtype, engine, A, B, transA=False, transB=False, aop=0, epi=0, C0=None, C20=None,
             mask=None, nan=0, splits=0, a_dtype=-1, b_dtype=-1, pad_a=0, pad_b=0, pad_c=0, off_a=0, off_b=0, off_c=0,
             ws_bytes=None, info=None):
    """C = epi(aop(op(A)) @ op(B)) through skf_gemm; A/B given as stored (row-major).  pad_* : extra elements per row of the
    stored operand / result, off_* : elements by which its pointer is advanced into a larger upload (the pads of C, C2 and
    the mask hold NaN / 0xFF and must come back bit for bit).  `info` (a dict) receives the product of the operands as stored
    in extended precision ('P') and of their magnitudes ('absP'), for the elementwise bound (K + s) u |A| |B|."""
    npd = nat.NP_DTYPE[dtype]
    A = np.ascontiguousarray(A, dtype=npd if a_dtype < 0 else nat.NP_DTYPE[a_dtype])
    B = np.ascontiguousarray(B, dtype=npd if b_dtype < 0 else nat.NP_DTYPE[b_dtype])
    M, K = (A.shape[1], A.shape[0]) if transA else A.shape
    N = B.shape[0] if transB else B.shape[1]
    mem = rt.mem
    a, b = Stored(mem, A, pad_a, off_a), Stored(mem, B, pad_b, off_b)
    Cm = np.zeros((M, N), npd) if C0 is None else np.array(C0, dtype=npd)
    C2m = np.zeros((M, N), npd) if C20 is None else np.array(C20, dtype=npd)
    c, c2 = Stored(mem, Cm, pad_c, off_c), Stored(mem, C2m, pad_c, off_c)
    d = nat.GemmDesc()
    d.A, d.B, d.C, d.C2 = a.ptr, b.ptr, c.ptr, c2.ptr
    d.sa_m, d.sa_k = (1, a.ld) if transA else (a.ld, 1)
    d.sb_k, d.sb_n = (1, b.ld) if transB else (b.ld, 1)
    d.ldc = d.ldc2 = c.ld
    d.M, d.N, d.K = M, N, K
    d.aop, d.epi, d.nan_to_num, d.splits = aop, epi, nan, splits
    d.a_dtype, d.b_dtype = a_dtype, b_dtype
    keep = None
    if mask is not None:                    # the stand-alone operator takes one byte per entry
        keep = Stored(mem, np.ascontiguousarray(mask, dtype=np.uint8), pad_c, off_c)
        d.mask, d.ldmask = keep.ptr, keep.ld
    ws = mem.empty(64 * M * N * 8 + 256 if ws_bytes is None else ws_bytes)
    rt.call('skf_gemm', dtype, engine, C.byref(d), ws.ptr, ws.nbytes, None)
    if keep is not None:
        keep.download()
    if info is not None:
        wide = np.longdouble if dtype == nat.SKF_F64 else np.float64
        Aw, Bw = (A.T if transA else A).astype(wide), (B.T if transB else B).astype(wide)
        with np.errstate(invalid='ignore', over='ignore'):
            info['P'], info['absP'] = Aw @ Bw, np.abs(Aw) @ np.abs(Bw)
        info['u'] = 2.0 ** -53 if dtype == nat.SKF_F64 else 2.0 ** -24
    return c.download(), c2.download()


SHAPES = [(1, 1, 1), (5, 3, 7), (50, 10, 100), (64, 64, 32), (70, 130, 33), (129, 200, 65),
          (200, 129, 17), (33, 260, 40)]


@pytest.mark.parametrize('dtype', [nat.SKF_F64, nat.SKF_F32])
@pytest.mark.parametrize('engine', [nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU])
@pytest.mark.parametrize('shape', SHAPES)
def test_gemm_plain_all_layouts(rt, dtype, engine, shape):
    M, N, K = shape
    rs = np.random.RandomState(M * 1000 + N * 10 + K)
    tol = 1e-13 if dtype == nat.SKF_F64 else 2e-6
    for transA in (False, True):
        for transB in (False, True):
            A = rs.randn(*((K, M) if transA else (M, K)))
            B = rs.randn(*((N, K) if transB else (K, N)))       # asymmetric operands
            got, _ = run_gemm(rt, dtype, engine, A, B, transA, transB)
            want = (A.T if transA else A) @ (B.T if transB else B)
            assert relerr(got, want) < tol, (transA, transB)


@pytest.mark.parametrize('dtype', [nat.SKF_F64, nat.SKF_F32])
@pytest.mark.parametrize('engine', [nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU])
def test_gemm_epilogues_and_operand_ops(rt, dtype, engine):
    rs = np.random.RandomState(5)
    M, N, K = 70, 45, 90
    tol = 1e-13 if dtype == nat.SKF_F64 else 2e-6
    A, B = rs.randn(M, K), rs.randn(K, N)
    C0, C20 = rs.rand(M, N), rs.rand(M, N)
    P = A @ B
    got, _ = run_gemm(rt, dtype, engine, A, B, epi=1, C0=C0)
    assert relerr(got, C0 + P) < tol
    g1, g2 = run_gemm(rt, dtype, engine, A, B, epi=2, C0=C0, C20=C20)
    assert relerr(g1, np.maximum(P, 0)) < tol and relerr(g2, np.maximum(-P, 0)) < tol
    g1, g2 = run_gemm(rt, dtype, engine, A, B, epi=3, C0=C0, C20=C20)
    assert relerr(g1, C0 + np.maximum(P, 0)) < tol and relerr(g2, C20 + np.maximum(-P, 0)) < tol
    mask = rs.rand(M, N) > 0.6
    got, _ = run_gemm(rt, dtype, engine, A, B, epi=4, C0=C0, mask=mask)
    assert relerr(got, np.where(mask, P, C0)) < tol
    got, _ = run_gemm(rt, dtype, engine, A, B, aop=1)
    assert relerr(got, np.maximum(A, 0) @ B) < tol
    got, _ = run_gemm(rt, dtype, engine, A, B, aop=2)
    assert relerr(got, np.maximum(-A, 0) @ B) < tol


@pytest.mark.parametrize('dtype', [nat.SKF_F64, nat.SKF_F32])
def test_gemm_split_k_and_nan_to_num(rt, dtype):
    rs = np.random.RandomState(6)
    tol = 1e-13 if dtype == nat.SKF_F64 else 3e-6
    A, B = rs.randn(700, 20), rs.randn(700, 30)          # Gram-like: K = 700, tiny output
    want = A.T @ B
    for splits in (0, 1, 3, 7):
        got, _ = run_gemm(rt, dtype, nat.SKF_ENGINE_MFMA, A, B, transA=True, splits=splits)
        assert relerr(got, want) < tol, splits
    g1, g2 = run_gemm(rt, dtype, nat.SKF_ENGINE_MFMA, A, B, transA=True, splits=4, epi=3,
                      C0=np.ones((20, 30)), C20=np.ones((20, 30)))
    assert relerr(g1, 1 + np.maximum(want, 0)) < tol and relerr(g2, 1 + np.maximum(-want, 0)) < tol
    A2 = A.copy()
    A2[3, 2] = np.nan
    A2[5, 4] = np.inf
    got, _ = run_gemm(rt, dtype, nat.SKF_ENGINE_MFMA, A2, B, transA=True, nan=1, splits=2)
    with np.errstate(invalid='ignore'):
        ref = np.nan_to_num((A2.T @ B).astype(nat.NP_DTYPE[dtype]))
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got[2] == 0, ref[2] == 0)
    assert relerr(np.delete(got, [2, 4], axis=0), np.delete(ref, [2, 4], axis=0)) < tol


@pytest.mark.parametrize('engine', [nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU])
def test_gemm_mixed_operand_types(rt, engine):
    """f32 operands with f64 arithmetic (Gram / G^T P) and f32 x f64 -> f32 (P S^T, G B)."""
    rs = np.random.RandomState(8)
    G = rs.rand(900, 40).astype(np.float32)
    P = rs.randn(900, 70).astype(np.float32)
    got, _ = run_gemm(rt, nat.SKF_F64, engine, G, P, transA=True, a_dtype=nat.SKF_F32, b_dtype=nat.SKF_F32)
    want = G.astype(np.float64).T @ P.astype(np.float64)
    assert got.dtype == np.float64 and relerr(got, want) < 1e-14
    S = rs.randn(40, 70)
    got, _ = run_gemm(rt, nat.SKF_F32, engine, P, S, transB=True, a_dtype=nat.SKF_F32, b_dtype=nat.SKF_F64)
    assert got.dtype == np.float32 and relerr(got, P.astype(np.float64) @ S.T) < 2e-6
    lib = rt.lib
    d = nat.GemmDesc()
    d.A = d.B = d.C = 1
    d.a_dtype, d.b_dtype = nat.SKF_F64, nat.SKF_F32
    d.M = d.N = d.K = 4
    assert lib.skf_gemm(nat.SKF_F32, engine, C.byref(d), None, 0, None) == -1


def bf16_result(rt, M, N, ldc_pad):
    """The f32 result of a bf16 operator: M rows N + ldc_pad apart, every element NaN before the call."""
    return Stored(rt.mem, np.full((M, N), np.nan, np.float32), ldc_pad)


def bf16_check(got, Ar, Br, K, splits, what):
    """|got - want| <= 2 (K + s) 2^-24 (|A| |B|)_ij against the f64 product of the operands as stored (exact bf16 products,
    f32 accumulation in any order, the slice sum; the factor 2: the matrix core's alignment of a 32-term step)."""
    want, absP = Ar @ Br, np.abs(Ar) @ np.abs(Br)
    elementwise(got, want, 2.0 * (K + max(splits, 1)) * 2.0 ** -24 * absP, what)
    return want


def run_gemm_bf16(rt, A, B, splits=0, ldc_pad=0, lda_pad=0, ws_bytes=None, check=None):
    """C = A @ B with bf16 operands through skf_gemm_bf16 (A: M x K, B: K x N given as floats).  ldc_pad: extra elements per
    row of C (NaN before and after), lda_pad: extra (zero) elements per row of A, a multiple of 8; `check`: a label -- hold
    the result to the elementwise bound of bf16_check."""
    M, K = A.shape
    N = B.shape[1]
    Kp = (K + 63) // 64 * 64
    Ab = np.zeros((M, Kp + lda_pad), np.uint16)
    Ab[:, :K] = nat.to_bf16_bits(A)
    Bb = np.zeros((N, Kp), np.uint16)
    Bb[:, :K] = nat.to_bf16_bits(B.T)
    a, b = rt.mem.from_host(Ab), rt.mem.from_host(Bb)
    c = bf16_result(rt, M, N, ldc_pad)
    ws = rt.mem.empty(40 * M * N * 4 + 256 if ws_bytes is None else ws_bytes)
    rt.call('skf_gemm_bf16', a.ptr, Kp + lda_pad, b.ptr, Kp, c.ptr, c.ld, M, N, Kp, splits, ws.ptr, ws.nbytes, None)
    got = c.download()
    Ar, Br = nat.from_bf16_bits(Ab[:, :K]).astype(np.float64), nat.from_bf16_bits(Bb[:, :K]).astype(np.float64).T
    want = Ar @ Br if check is None else bf16_check(got, Ar, Br, K, splits, check)
    return got, want


@pytest.mark.parametrize('shape', [(1, 1, 1), (16, 16, 32), (128, 128, 64), (130, 100, 70), (257, 128, 200),
                                   (100, 256, 129), (200, 200, 500), (129, 300, 64),
                                   (4100, 128, 70), (4200, 256, 200), (4097, 300, 64), (4100, 48, 200)])
def test_gemm_bf16_contraction(rt, shape):
    """Both workgroup shapes: the 128-row register-staged kernel (M < 4096) and the 256-row LDS-DMA
    kernel with its 3-deep ring and scheduled DMA pieces (M >= 4096); row / column / K tails, split-K."""
    M, N, K = shape
    rs = np.random.RandomState(M + N + K)
    A, B = rs.randn(M, K), rs.randn(K, N)           # asymmetric operands
    for splits in ((0, 1, 3) if M < 4096 else (0, 2)):
        got, want = run_gemm_bf16(rt, A, B, splits)
        assert relerr(got, want) < 2e-6, splits     # exact products, f32 accumulation


def run_gemm_bf16_tn(rt, R, G, splits=0, ldc_pad=0, lda_pad=0, ws_bytes=None, check=None):
    """Q = R^T @ G through skf_gemm_bf16_tn: R (K x M, row-major, the relation as stored) is read
    transposed out of LDS; G (K x N) is passed as the stored transpose G^T."""
    K, M = R.shape
    N = G.shape[1]
    Kp = (K + 63) // 64 * 64
    lda = (M + 63) // 64 * 64 + lda_pad
    Rb = np.zeros((Kp, lda), np.uint16)
    Rb[:K, :M] = nat.to_bf16_bits(R)
    Gt = np.zeros((N, Kp), np.uint16)
    Gt[:, :K] = nat.to_bf16_bits(G.T)
    a, b = rt.mem.from_host(Rb), rt.mem.from_host(Gt)
    c = bf16_result(rt, M, N, ldc_pad)
    ws = rt.mem.empty(40 * M * N * 4 + 256 if ws_bytes is None else ws_bytes)
    rt.call('skf_gemm_bf16_tn', a.ptr, lda, b.ptr, Kp, c.ptr, c.ld, M, N, Kp, splits, ws.ptr, ws.nbytes, None)
    got = c.download()
    Ar, Br = nat.from_bf16_bits(Rb[:K, :M]).astype(np.float64).T, nat.from_bf16_bits(Gt[:, :K]).astype(np.float64).T
    want = Ar @ Br if check is None else bf16_check(got, Ar, Br, K, splits, check)
    return got, want


@pytest.mark.parametrize('shape', [(1, 1, 1), (16, 16, 32), (64, 128, 64), (100, 130, 70), (200, 257, 128),
                                   (129, 100, 256), (500, 200, 200), (64, 129, 300), (300, 520, 100), (200, 300, 40)])
def test_gemm_bf16_transposed_a(rt, shape):
    """Q = R^T G_i from the row-major relation: LDS-DMA of [64 k][256 m] tiles, ds_read_b64_tr_b16 fragments
    (emulated with the lane map measured on the hardware); K x M x N with tails everywhere, split-K."""
    K, M, N = shape
    rs = np.random.RandomState(M + N + K)
    R, G = rs.randn(K, M), rs.randn(K, N)           # asymmetric: a transposed or mis-swizzled read cannot pass
    for splits in (0, 1, 2):
        got, want = run_gemm_bf16_tn(rt, R, G, splits)
        assert relerr(got, want) < 2e-6, splits


def run_gemm_bits(rt, Rb, G, transposed, splits=0, ldc_pad=0, ws_bytes=None, check=None):
    """Binary relation Rb (0 / 1) as a bitmap through skf_gemm_bits: P = Rb @ G (transposed=0, Rb is M x K) or
    Q = Rb^T @ G (transposed=1, Rb is K x M)."""
    rows, cols = Rb.shape
    ldb_bytes = (cols + 63) // 64 * 8
    rows_pad = (rows + 63) // 64 * 64
    bits = np.zeros((rows_pad, ldb_bytes), np.uint8)
    bits[:rows, :(cols + 7) // 8] = np.packbits(Rb.astype(bool), axis=1, bitorder='little')
    if transposed:
        K, M = rows, cols
        Kp = rows_pad
    else:
        M, K = rows, cols
        Kp = ldb_bytes * 8
    N = G.shape[1]
    Gt = np.zeros((N, Kp), np.uint16)
    Gt[:, :K] = nat.to_bf16_bits(G.T)
    a, b = rt.mem.from_host(bits), rt.mem.from_host(Gt)
    c = bf16_result(rt, M, N, ldc_pad)
    ws = rt.mem.empty(40 * M * N * 4 + 256 if ws_bytes is None else ws_bytes)
    rt.call('skf_gemm_bits', a.ptr, ldb_bytes, b.ptr, Kp, c.ptr, c.ld, M, N, Kp, 1 if transposed else 0, splits,
            ws.ptr, ws.nbytes, None)
    got = c.download()
    Ar, Br = (Rb.T if transposed else Rb).astype(np.float64), nat.from_bf16_bits(Gt[:, :K]).astype(np.float64).T
    want = Ar @ Br if check is None else bf16_check(got, Ar, Br, K, splits, check)
    return got, want


@pytest.mark.parametrize('shape', [(1, 1, 1), (70, 100, 130), (128, 200, 257), (256, 129, 100), (200, 500, 200),
                                   (300, 64, 129), (100, 300, 520), (33, 260, 200)])
@pytest.mark.parametrize('transposed', [0, 1])
def test_gemm_bits_binary_relation_as_a_bitmap(rt, shape, transposed):
    """A 0 / 1 relation stored as one bit per entry, expanded to bf16 in LDS between the MFMA groups: both
    contractions (rows of the bitmap as output rows, or as the contraction index with transposed fragment
    reads), N <= 128 and N > 128 (3- and 2-deep G^T rings), tails everywhere, split-K."""
    N, rows, cols = shape
    rs = np.random.RandomState(rows + cols + N + transposed)
    Rb = (rs.rand(rows, cols) < 0.3).astype(np.float64)
    G = rs.randn(rows if transposed else cols, N)
    for splits in (0, 1, 2):
        got, want = run_gemm_bits(rt, Rb, G, transposed, splits)
        assert relerr(got, want) < 2e-6, splits


def test_to_bf16_and_transpose(rt):
    rs = np.random.RandomState(2)
    X = rs.randn(70, 45)
    for src_dtype, npd in ((nat.SKF_F64, np.float64), (nat.SKF_F32, np.float32)):
        src = rt.mem.from_host(X.astype(npd))
        dst = rt.mem.from_host(np.zeros((70, 64), np.uint16))
        rt.call('skf_to_bf16', dst.ptr, 64, src_dtype, src.ptr, 45, 70, 45, 0, None)
        got = rt.mem.to_host(dst, (70, 64), np.uint16)
        np.testing.assert_array_equal(got[:, :45], nat.to_bf16_bits(X.astype(npd)))
        assert (got[:, 45:] == 0).all()
        dstT = rt.mem.from_host(np.zeros((45, 128), np.uint16))
        rt.call('skf_to_bf16', dstT.ptr, 128, src_dtype, src.ptr, 45, 70, 45, 1, None)
        gotT = rt.mem.to_host(dstT, (45, 128), np.uint16)
        np.testing.assert_array_equal(gotT[:, :70], nat.to_bf16_bits(X.astype(npd)).T)
        assert (gotT[:, 70:] == 0).all()


def run_pinv(rt, dtype, A, route=None):
    npd = nat.NP_DTYPE[dtype]
    n = A.shape[0]
    need = C.c_size_t()
    rt.call('skf_pinv_sym_workspace_bytes', n, C.byref(need))
    a = rt.mem.from_host(np.ascontiguousarray(A, dtype=npd))
    k = rt.mem.empty(n * n * np.dtype(npd).itemsize)
    ws = rt.mem.empty(need.value)
    rt.call('skf_pinv_sym', dtype, a.ptr, n, k.ptr, n, n, ws.ptr, need.value, None)
    if route is not None:
        # the verdict word of the operator's workspace (skf_pinv_sym: three n_pad^2 f64 matrices, the eigenvalue row, then
        # int words: order, original order at +16, verdict at +32): 1 = an inverse written straight into K (fast path, or
        # the multi-workgroup deflation), 2 = the one-workgroup deflation, 0 = the eigen-solver
        npad = (n + 1) // 2 * 2
        mat = (npad * npad * 8 + 255) // 256 * 256
        off = 3 * mat + (npad * 8 + 255) // 256 * 256 + 32 * 4
        words = rt.mem.to_host(ws, (need.value // 4,), np.int32)
        route.append(int(words[off // 4]))
    return rt.mem.to_host(k, (n, n), npd)


@pytest.mark.parametrize('n', [1, 2, 5, 10, 31, 32, 33, 50, 70])
def test_pinv_full_rank_matches_scipy(rt, n, monkeypatch=None):
    """All routes: blocked Cholesky (default), plain Cholesky, Jacobi eigen-solver (forced)."""
    import os
    import scipy.linalg as spla
    rs = np.random.RandomState(n)
    G = rs.rand(4 * n + 3, n)
    A = G.T @ G
    want = spla.pinv(A)
    for env in ({}, {'SKF_CHOL_UNBLOCKED': '1'}, {'SKF_PINV_JACOBI': '1'}):
        if env.get('SKF_PINV_JACOBI') and n > 50:
            continue
        os.environ.update(env)
        try:
            got = run_pinv(rt, nat.SKF_F64, A)
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert relerr(got, want) < 1e-9 * max(1.0, np.linalg.cond(A) * 1e-3), env
        assert relerr(A @ got @ A, A) < 1e-11


@pytest.mark.parametrize('n', [65, 96, 130, 200, 256])
def test_pinv_blocked_sweep_orders_65_to_256(rt, n):
    """Orders 65 .. 256 take the blocked sweep operator (sweep_inverse_kernel: K written by the kernel itself): against
    scipy and against the blocked Cholesky inverse it replaced (SKF_PINV_SWEEP=0), badly scaled columns included (the pivot
    test is relative to each pivot's own diagonal entry, as in the Cholesky kernels); a singular matrix is declined and
    lands on the deflation path with the same result as before."""
    import os
    import scipy.linalg as spla
    rs = np.random.RandomState(n)
    G = rs.rand(3 * n + 5, n)
    A = G.T @ G
    want = spla.pinv(A)
    got = run_pinv(rt, nat.SKF_F64, A)
    os.environ['SKF_PINV_SWEEP'] = '0'
    try:
        old = run_pinv(rt, nat.SKF_F64, A)
    finally:
        os.environ.pop('SKF_PINV_SWEEP', None)
    assert relerr(got, want) < 1e-9 * max(1.0, np.linalg.cond(A) * 1e-3)
    assert relerr(got, old) < 1e-9 * max(1.0, np.linalg.cond(A) * 1e-3)
    assert relerr(A @ got @ A, A) < 1e-11
    assert np.abs(got - got.T).max() <= 1e-12 * np.abs(got).max()
    if n in (96, 200):
        scale = 10.0 ** (-4.0 * rs.rand(n))
        Gs = rs.rand(4 * n, n) * scale
        As = Gs.T @ Gs
        d = np.sqrt(np.diag(As))
        gs = run_pinv(rt, nat.SKF_F64, As)
        # (cond(As) ~ 4e9: scipy's own inverse is off by 1e-8 there; the equilibrated matrix has cond ~ 2e3 and its inverse,
        # scaled back, is the reference -- the sweep is within 1e-13 of it, the Cholesky inverse within 3e-14)
        W = np.outer(d, d)
        assert relerr(gs * W, np.linalg.inv(As / W)) < 1e-12
        Gd = rs.rand(n // 2, n)                        # rank n / 2: the sweep meets a failed pivot and hands over
        Ad = Gd.T @ Gd
        assert relerr(run_pinv(rt, nat.SKF_F64, Ad), spla.pinv(Ad)) < 1e-7


@pytest.mark.parametrize('n', [65, 96, 130, 200, 256])
def test_pinv_sweep_one_launch_per_block_step_keeps_the_bits(rt, n):
    """sweep_step_kernel (round 5: one launch per block step, the rank-32 update of a step spread over row slabs, the matrix
    alternating between two copies) against sweep_inverse_kernel (one workgroup, in place): every element takes the same
    arithmetic in the same order, so the inverses are equal bit for bit -- at slabs of 32 and 64 rows, with a ragged last
    block, and for a matrix that fails a pivot in a late step (both hand over to the deflation)."""
    import os
    rs = np.random.RandomState(100 + n)
    G = rs.rand(3 * n + 5, n)
    A = G.T @ G
    Gd = np.concatenate([rs.rand(n - 7, n - 7), np.zeros((n - 7, 7))], axis=1)     # pivots fail in the LAST block
    Gd[:, -7:] = Gd[:, :7]
    Ad = Gd.T @ Gd

    def run(step_min, rows=None):
        os.environ['SKF_SWEEP_STEP_MIN'] = str(step_min)
        if rows:
            os.environ['SKF_SWEEP_ROWS'] = str(rows)
        try:
            return run_pinv(rt, nat.SKF_F64, A), run_pinv(rt, nat.SKF_F64, Ad)
        finally:
            os.environ.pop('SKF_SWEEP_STEP_MIN', None)
            os.environ.pop('SKF_SWEEP_ROWS', None)

    one, one_d = run(0)
    for rows in (32, 64):
        stepped, stepped_d = run(65, rows)
        assert np.array_equal(one, stepped), rows
        assert np.array_equal(one_d, stepped_d), rows
    assert relerr(A @ one @ A, A) < 1e-11


@pytest.mark.parametrize('n', [257, 300, 420])
def test_pinv_blocked_sweep_above_order_256(rt, n):
    """Orders above 256 (round 5): the step-per-launch sweep with the column operands of the update read from the matrix in
    memory (sweep_step_kernel<true>; the LDS holds the pivot rows and the slab's rows only) against scipy and against the
    blocked Cholesky inverse it replaces there (SKF_SWEEP_BIG=0); a matrix that fails a pivot is handed to the deflation."""
    import os
    import scipy.linalg as spla
    rs = np.random.RandomState(n)
    G = rs.rand(3 * n + 5, n)
    A = G.T @ G
    got = run_pinv(rt, nat.SKF_F64, A)
    os.environ['SKF_SWEEP_BIG'] = '0'
    try:
        old = run_pinv(rt, nat.SKF_F64, A)
    finally:
        os.environ.pop('SKF_SWEEP_BIG', None)
    want = spla.pinv(A)
    bound = 1e-9 * max(1.0, np.linalg.cond(A) * 1e-3)
    assert relerr(got, want) < bound and relerr(got, old) < bound
    assert relerr(A @ got @ A, A) < 1e-11
    assert np.abs(got - got.T).max() <= 1e-12 * np.abs(got).max()
    if n == 300:
        Gd = rs.rand(n - 40, n)                        # rank n - 40: a pivot of the last blocks fails
        Ad = Gd.T @ Gd
        assert relerr(run_pinv(rt, nat.SKF_F64, Ad), spla.pinv(Ad)) < 1e-7


def test_pinv_rank_deficient_truncates_like_scipy(rt):
    """reference tests/test_n_run.py:14: rank 50 factor of 30 objects -> Gram has rank 30."""
    import scipy.linalg as spla
    rs = np.random.RandomState(1)
    G = rs.rand(30, 50)
    A = G.T @ G
    got = run_pinv(rt, nat.SKF_F64, A)
    want = spla.pinv(A)
    assert np.abs(got).max() < 10 * np.abs(want).max()
    assert relerr(got, want) < 1e-7
    got32 = run_pinv(rt, nat.SKF_F32, A)
    assert np.isfinite(got32).all()


@pytest.mark.parametrize('n,rank', [(50, 30), (96, 40), (130, 65), (33, 1)])
def test_pinv_deflation_matches_scipy_and_the_eigen_path(rt, n, rank, monkeypatch):
    """A rank-deficient Gram matrix with a clear spectral gap goes through the rank-revealing deflation
    (pivoted Cholesky, A^+ = Y Y^T with Y = L (L^T L)^-1): same result as scipy.linalg.pinv and as the Jacobi
    eigen path with its exact cut-off (SKF_PINV_JACOBI=1), duplicate columns included."""
    import scipy.linalg as spla
    rs = np.random.RandomState(n + rank)
    G = rs.rand(rank, n)
    G[:, n // 2] = G[:, 1]                       # an exactly duplicated latent column
    A = G.T @ G
    want = spla.pinv(A)
    got = run_pinv(rt, nat.SKF_F64, A)
    assert relerr(got, want) < 1e-8
    monkeypatch.setenv('SKF_PINV_JACOBI', '1')
    exact = run_pinv(rt, nat.SKF_F64, A)
    assert relerr(got, exact) < 1e-8


@pytest.mark.parametrize('n,rank', [(300, 170), (420, 97), (260, 259)])
def test_pinv_deflation_over_several_workgroups_above_order_256(rt, n, rank, monkeypatch):
    """Round 6: above order 256 a rank-deficient Gram matrix is deflated by pchol_step_kernel -- one launch per block of
    up to 32 pivots over slabs of 64 rows, pivots rejected inside a block when the block's earlier pivots took them to the
    noise level (a duplicated column is chosen twice by the stale diagonal) --, B = L^T L is inverted by the blocked sweep of
    the fast path and K = Y Y^T leaves two gated products: same result as scipy.linalg.pinv and as the one-workgroup
    kernel (SKF_SWEEP_BIG=0 switches the multi-workgroup route off with the fast path it builds on)."""
    import scipy.linalg as spla
    rs = np.random.RandomState(n + rank)
    G = rs.rand(rank, n)
    G[:, n // 2] = G[:, 1]                       # an exactly duplicated latent column
    G[:, 7] = 0.0                                # and an all-zero one
    A = G.T @ G
    want = spla.pinv(A)
    route = []
    got = run_pinv(rt, nat.SKF_F64, A, route)
    assert route == [1]                          # written straight into K by the multi-workgroup route
    assert relerr(got, want) < 1e-8, relerr(got, want)
    assert relerr(A @ got @ A, A) < 1e-10
    assert np.abs(got - got.T).max() <= 1e-10 * np.abs(got).max()
    monkeypatch.setenv('SKF_SWEEP_BIG', '0')
    one_wg = run_pinv(rt, nat.SKF_F64, A, route)
    assert route == [1, 2]                       # ... and by the one-workgroup kernel (eigen format) without it
    assert relerr(got, one_wg) < 1e-8


def test_pinv_ambiguous_spectrum_above_order_256_is_left_to_the_exact_cut_off(rt):
    """The multi-workgroup deflation applies the same gap test: an accepted pivot inside (1e-10, 1e-7) of the largest
    declines the matrix, and the eigen path with scipy's cut-off takes it."""
    import scipy.linalg as spla
    rs = np.random.RandomState(5)
    n = 258
    Qm, _ = np.linalg.qr(rs.randn(n, n))
    w = np.array([1.0] * 40 + [1e-8] * 2 + [0.0] * (n - 42))
    A = (Qm * w) @ Qm.T
    A = 0.5 * (A + A.T)
    route = []
    got = run_pinv(rt, nat.SKF_F64, A, route)
    assert route == [0]                           # declined by both deflations: the eigen-solver
    want = spla.pinv(A)
    assert np.abs(got).max() > 1e6                # the 1e-8 directions were inverted, not dropped
    assert relerr(got, want) < 1e-6


def test_pinv_ambiguous_spectrum_falls_back_to_the_exact_cut_off(rt):
    """A singular value inside the deflation's gap band (1e-10 .. 1e-7 of the largest) is neither noise nor safely
    invertible by a pivot rule: the deflation declines and the eigen path applies scipy's cut-off (which keeps
    it: 1e-8 is far above n * eps)."""
    import scipy.linalg as spla
    rs = np.random.RandomState(4)
    Qm, _ = np.linalg.qr(rs.randn(24, 24))
    w = np.array([1.0] * 10 + [1e-8] * 2 + [0.0] * 12)
    A = (Qm * w) @ Qm.T
    A = 0.5 * (A + A.T)
    got = run_pinv(rt, nat.SKF_F64, A)
    want = spla.pinv(A)
    assert np.abs(got).max() > 1e7                # the 1e-8 directions were inverted, not dropped
    assert relerr(got, want) < 1e-6


@pytest.mark.parametrize('n', [12, 40, 70])
def test_pinv_badly_scaled_columns_match_scipy(rt, n):
    """Latent dimensions of very different scale (column norms down to 1e-5 of the largest: diagonal of
    the Gram matrix spread over 1e-10) but independent: the pivot test of the Cholesky fast path is
    relative to each pivot's own diagonal, so these stay on it; scipy inverts them too (sigma_min /
    sigma_max ~ 1e-10 is far above its cut-off).  Compared in the equilibrated metric."""
    import os
    import scipy.linalg as spla
    rs = np.random.RandomState(n)
    scale = 10.0 ** (-5.0 * rs.rand(n))
    scale[0], scale[-1] = 1.0, 1e-5
    G = rs.rand(6 * n, n) * scale
    A = G.T @ G
    want = spla.pinv(A)
    d = np.sqrt(np.diag(A))
    for env in ({}, {'SKF_CHOL_NO_SMALL': '1'}, {'SKF_CHOL_UNBLOCKED': '1'}):
        os.environ.update(env)
        try:
            got = run_pinv(rt, nat.SKF_F64, A)
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert relerr(got * np.outer(d, d), want * np.outer(d, d)) < 1e-8, env


def test_pinv_zero_and_diagonal(rt):
    got = run_pinv(rt, nat.SKF_F64, np.zeros((6, 6)))
    assert (got == 0).all()
    d = np.diag([4.0, 2.0, 0.0, 1e-30, 5.0])
    got = run_pinv(rt, nat.SKF_F64, d)
    np.testing.assert_allclose(got, np.diag([0.25, 0.5, 0.0, 0.0, 0.2]), atol=1e-15)


STRIDED = [(nat.SKF_F64, 33, None, 40, 37), (nat.SKF_F64, 33, 20, 40, 37), (nat.SKF_F32, 33, None, 40, 37),
           (nat.SKF_F32, 33, 20, 40, 37), (nat.SKF_F64, 70, None, 70, 72)]


@pytest.mark.parametrize('dtype,n,rank,lda,ldk', STRIDED)
def test_pinv_with_leading_dimensions_above_the_order(rt, dtype, n, rank, lda, ldk):
    """The stand-alone operator on a matrix stored with lda > n into a K with ldk > n, in both element types (pack and both
    unpack kernels with the caller's strides; tests/pinv_cases.py).  ldk != n rules out the sweep, which writes a dense f64 K
    itself: the full-rank matrix takes the Cholesky inverse + unpack (verdict 1), the rank-20 one the one-workgroup deflation +
    eigen unpack (verdict 2).  Order 70 is the smallest at which ldk alone decides: six launches (pack, Cholesky, unpack,
    deflation, eigen-solver, eigen unpack) with ldk = 72 against the sweep's 4 + ceil(70 / 32) with ldk = 70.  Against
    scipy.linalg.pinv under the bounds of test_pinv_full_rank_matches_scipy / test_pinv_deflation_matches_scipy_and_the_eigen_path,
    f32 scaled by eps_f32 / eps_f64 (the inputs are exact in f32; measured on the emulator: f64 3.7e-15 / 1.6e-14 / 9.5e-15,
    f32 2.6e-8 / 2.6e-8).  Columns n .. ldk - 1 of K keep the bytes they had."""
    import scipy.linalg as spla
    import pinv_cases
    A = pinv_cases.strided_matrix(n, rank)
    want = spla.pinv(A)
    got, pad, verdict, launches = pinv_cases.run_pinv_strided(rt, dtype, A, lda, ldk)
    bound = 1e-9 * max(1.0, np.linalg.cond(A) * 1e-3) if rank is None else 1e-8
    if dtype == nat.SKF_F32:
        bound *= float(np.finfo(np.float32).eps) / float(np.finfo(np.float64).eps)
    err = relerr(got.astype(np.float64), want)
    print('pinv n=%d rank=%s lda=%d ldk=%d dtype=%d: %.3e (bound %.3e), verdict %d, %d launches' % (n, rank, lda, ldk, dtype, err, bound, verdict, launches))
    assert err < bound
    assert (pad == pinv_cases.POISON).all()
    assert verdict == (1 if rank is None else 2)
    assert launches == 6
    if n == 70:
        dense = pinv_cases.run_pinv_strided(rt, dtype, A, lda, n)
        assert dense[2] == 1 and dense[3] == 4 + (n + 31) // 32
        assert relerr(dense[0], want) < bound


def test_fill_uniform_matches_oracle_hash(rt):
    from oracle.dfmf_oracle import hash_uniform_matrix
    for dtype, npd in ((nat.SKF_F64, np.float64), (nat.SKF_F32, np.float32)):
        buf = rt.mem.empty(37 * 53 * 8)
        rt.call('skf_fill_uniform', dtype, buf.ptr, 37, 53, 53, 9, 1.0, 0.0, None)
        got = rt.mem.to_host(buf, (37, 53), npd)
        np.testing.assert_array_equal(got, hash_uniform_matrix(9, 37, 53).astype(npd))
    buf = rt.mem.empty(8 * 16 * 2)
    rt.call('skf_fill_uniform', nat.SKF_BF16, buf.ptr, 8, 16, 16, 3, 2.0, -1.0, None)
    got = rt.mem.to_host(buf, (8, 16), np.uint16)
    want = (hash_uniform_matrix(3, 8, 16) * 2.0 - 1.0).astype(np.float32)
    back = (got.astype(np.uint32) << 16).view(np.float32)
    assert np.abs(back - want).max() <= np.abs(want).max() * 2 ** -8


def test_errors_are_reported_not_thrown(rt):
    lib = rt.lib
    assert lib.skf_gemm(nat.SKF_F32, 0, None, None, 0, None) == -1
    assert b'null' in lib.skf_last_error()
    with pytest.raises(nat.SkfNativeError):
        rt.call('skf_pinv_sym', nat.SKF_F64, None, 1, None, 1, 4, None, 0, None)
    out = nat._P()
    t = (nat.TypeDesc * 1)()
    t[0].n_obj, t[0].rank = 5, 0
    opt = nat.Options(nat.SKF_F64, nat.SKF_DFMF, -1, 0)
    assert lib.skf_plan_create(1, t, 0, None, 0, None, C.byref(opt), C.byref(out)) == -1


# ---- the stand-alone operators at the layouts the ABI promises: unpacked strides, misaligned bases, sub-matrix views, exact
# scratch, many slices (the GPU twins: tests/test_gpu_parity.py).  Reference and bound of every check below: the product of
# the operands AS STORED (rounded to f32 / bf16 first) in f64 (np.longdouble for the f64 engine), elementwise
#     |got - want| <= (K + s) u (|A| |B|)_ij          f32 / f64 products, u = 2^-24 / 2^-53, s the slice count
#     |got - want| <= 2 (K + s) 2^-24 (|A| |B|)_ij    bf16 products
# -- the first-order bound of a length-K sum in any order plus the sum of the slices; the factor 2 of the bf16 form covers the
# matrix core's internal alignment of a 32-term step (a derived allowance, not a measured one).
def slices_of(K, splits, bk):
    """The K slices a request for `splits` becomes (fit_slices of skf_gemm_launch.inc: whole K tiles of `bk` per slice)."""
    ktiles = -(-K // bk)
    chunk = -(-ktiles // max(min(splits, ktiles), 1)) * bk
    return -(-K // chunk)


def gemm_check(rt, dtype, engine, A, B, what, splits=0, epi=0, ones=False, mask=None, nan=0, skip_rows=(), s=None, **kw):
    """One skf_gemm call held to the elementwise bound (plain store; epi 3 on ones; epi 4 through a mask); `s`: the slices
    that run where they differ from the `splits` asked for."""
    M = A.shape[1] if kw.get('transA') else A.shape[0]
    N = B.shape[0] if kw.get('transB') else B.shape[1]
    info = {}
    C0 = np.ones((M, N)) if ones else (np.full((M, N), 0.25) if mask is not None else None)
    g1, g2 = run_gemm(rt, dtype, engine, A, B, epi=epi, C0=C0, C20=C0 if ones else None, mask=mask, nan=nan, splits=splits,
                      info=info, **kw)
    K = A.shape[0] if kw.get('transA') else A.shape[1]
    P, u = info['P'], info['u']
    bound = (K + max(splits if s is None else s, 1)) * u * info['absP']
    keep = np.setdiff1d(np.arange(M), skip_rows)
    if epi == 3:
        w1, w2 = 1 + np.maximum(P, 0), 1 + np.maximum(-P, 0)
        elementwise(g1[keep], w1[keep], bound[keep], what + ' C')
        elementwise(g2[keep], w2[keep], bound[keep], what + ' C2')
    elif epi == 4:
        elementwise(g1[keep], np.where(mask, P, 0.25)[keep], np.where(mask, bound, 0.0)[keep], what)
    else:
        elementwise(g1[keep], P[keep], bound[keep], what)
    return g1


def layouts(V):
    """(pad, off) of A, of B, pad and off of C: every operand layout with its like, and the pairs that differ in kind."""
    packed, unpacked, scalar, misaligned, view = (0, 0), (V, 0), (1, 0), (0, 1), (V, V)
    pairs = [(packed, packed), (unpacked, unpacked), (scalar, scalar), (misaligned, misaligned), (view, view),
             (unpacked, scalar), (scalar, unpacked), (misaligned, packed), (packed, misaligned), (view, unpacked)]
    return [(a, b, (0, 1, 3)[q % 3], (0, 0, 0, 1, V)[q % 5]) for q, (a, b) in enumerate(pairs)]


@pytest.mark.parametrize('dtype', [nat.SKF_F64, nat.SKF_F32])
@pytest.mark.parametrize('engine', [nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU])
def test_gemm_strides_and_alignment(rt, dtype, engine):
    """stage_mode (device) and host_stage_mode (host, which also decides the big tile) see strides, lengths and base
    alignment that do not coincide: V = 16 bytes of elements; operands packed, with V or 1 pad elements per row, one element
    off a 16-byte base, and as an aligned view into a wider matrix.  Pads of C hold NaN and come back bit for bit.

    Which tile a shape runs on (pick_tile, gemm_tile; matrix-core engine):
      K = 64, 64 + V   f32: (70, 40, .) the small tile (64 x 64 x 32, run-time modes), (130, 132, .) and (128 + V, 132, .) the
                       big tile (128 x 128 x 32, compile-time modes) where the layout pair has an instantiation.  f64: every
                       all-f64 product with 64 <= K <= 1024 takes the DEEP tile (32 x 32 x 64, run-time modes), so these
                       shapes reach neither the f64 small nor the f64 big tile.
      K = 48, 48 + V   below the deep tile's range: f64 (70, 40, .) runs the small tile (32 x 32 x 16), (130, 132, .) and
                       (64 + V, 132, .) the big tile (64 x 128 x 16; 64 + V: the row tail row_end - V of its 64 rows), with
                       host_stage_mode<double> deciding at V = 2; f32 takes its small / big tile with a partial K tile.
      K = 64 + V, 48 + V, M = 128 + V, 64 + V: the vector tails (k_end - V, row_end - V) on an unpacked stride.

    Against a mix-up of the stride test and the length test in stage_mode / host_stage_mode (s_row % V for K % V) the
    sharpness of this test rests on the emulator build alone: such a mix-up picks 16-byte loads for rows that start off a
    16-byte boundary, which return the right bytes on the hardware (the GPU twin cannot see it), while the host compiler's
    aligned 16-byte move faults on them and ends the emulator process."""
    V = 16 // np.dtype(nat.NP_DTYPE[dtype]).itemsize
    rs = np.random.RandomState(11)
    every = layouts(V)
    for (M, N, K), lays in (((70, 40, 64), every), ((130, 132, 64), every), ((70, 40, 64 + V), every[:5]),
                            ((128 + V, 132, 64), every[:5]), ((70, 40, 48), every), ((130, 132, 48), every),
                            ((70, 40, 48 + V), every[:5]), ((130, 132, 48 + V), every[:5]), ((64 + V, 132, 48), every[:5])):
        for transA in (False, True):
            for transB in (False, True):
                A = rs.randn(*((K, M) if transA else (M, K)))
                B = rs.randn(*((N, K) if transB else (K, N)))
                for (pa, oa), (pb, ob), pc, oc in lays:
                    what = 'gemm strides dtype %d engine %d %dx%dx%d tA %d tB %d A %d+%d B %d+%d C %d+%d' % (
                        dtype, engine, M, N, K, transA, transB, pa, oa, pb, ob, pc, oc)
                    gemm_check(rt, dtype, engine, A, B, what, transA=transA, transB=transB, pad_a=pa, off_a=oa, pad_b=pb,
                               off_b=ob, pad_c=pc, off_c=oc)


@pytest.mark.parametrize('dtype', [nat.SKF_F64, nat.SKF_F32])
def test_gemm_many_slices(rt, dtype):
    """splitk_reduce_z16_kernel (8 slices and more): A^T B with K = 1100, 8, 9 and 16 slices asked for on EXACTLY
    splits * M * N elements of scratch between guard bands -- plain store, the split accumulate on ones, the masked store
    with ldc = N + 3, nan_to_num.  A slice is a whole number of K tiles (slices_of): f64 (K tile 16) runs 8, 9 and 14
    slices, all on the z16 kernel; f32 (K tile 32, 35 tiles) runs 7 (splitk_reduce_kernel), 9 and 12 (z16).  The bound
    takes the slices that run."""
    from guarded import guarded
    rs = np.random.RandomState(12)
    A, B = rs.randn(1100, 20), rs.randn(1100, 30)
    M, N = 20, 30
    size = np.dtype(nat.NP_DTYPE[dtype]).itemsize
    mask = rs.rand(M, N) > 0.6
    A2 = A.copy()
    A2[3, 2], A2[5, 4] = np.nan, np.inf
    ran = [slices_of(1100, s, 16 if dtype == nat.SKF_F64 else 32) for s in (8, 9, 16)]
    assert ran == ([8, 9, 14] if dtype == nat.SKF_F64 else [7, 9, 12])
    with guarded(rt) as g:
        for splits, s in zip((8, 9, 16), ran):
            kw = dict(splits=splits, s=s, transA=True, ws_bytes=splits * M * N * size)
            what = 'gemm many slices dtype %d %d slices asked %d run' % (dtype, splits, s)
            gemm_check(g.rt, dtype, nat.SKF_ENGINE_MFMA, A, B, what + ' store', **kw)
            gemm_check(g.rt, dtype, nat.SKF_ENGINE_MFMA, A, B, what + ' epi 3', epi=3, ones=True, **kw)
            gemm_check(g.rt, dtype, nat.SKF_ENGINE_MFMA, A, B, what + ' epi 4', epi=4, mask=mask, pad_c=3, **kw)
            got = gemm_check(g.rt, dtype, nat.SKF_ENGINE_MFMA, A2, B, what + ' nan_to_num', nan=1, skip_rows=(2, 4), **kw)
            assert np.isfinite(got).all() and (got[2] == 0).all() and (np.abs(got[4]) == np.finfo(got.dtype).max).all()
    assert g.bands > 0


@pytest.mark.parametrize('op', ['plain', 'plain256', 'tn', 'bits0', 'bits1'])
def test_gemm_bf16_reduce_layouts(rt, op):
    """bf16_splitk_reduce_kernel off its 16-byte path: M * N odd (the scalar path with two slices and more), ldc = N + 3, an
    M * N % 4 == 0 product with ldc = N + 8, lda = Kp + 64 -- every run on exactly splits * M * N floats of scratch between
    guard bands.  The smallest shapes with two K tiles of 64 per slice and a row, a column and a K tail; (4097, 33, 200): the
    256-row kernel of the plain form."""
    from guarded import guarded
    rs = np.random.RandomState(13)

    def ws(M, N, s):
        return s * M * N * 4

    with guarded(rt) as g:
        r = g.rt
        if op in ('plain', 'plain256'):
            M, N, K = (129, 33, 200) if op == 'plain' else (4097, 33, 200)
            A, B = rs.randn(M, K), rs.randn(K, N)
            for s in ((2, 3) if op == 'plain' else (2,)):
                for pad in (0, 3):
                    run_gemm_bf16(r, A, B, s, ldc_pad=pad, ws_bytes=ws(M, N, s), check='bf16 %s %d slices ldc N + %d' % (op, s, pad))
            run_gemm_bf16(r, A, B, 2, lda_pad=64, ws_bytes=ws(M, N, 2), check='bf16 %s lda Kp + 64' % op)
            if op == 'plain':
                run_gemm_bf16(r, A, B[:, :32], 2, ldc_pad=8, ws_bytes=ws(M, 32, 2), check='bf16 plain 129 x 32 ldc N + 8')
        elif op == 'tn':
            K, M, N = 200, 129, 33
            R, G = rs.randn(K, M), rs.randn(K, N)
            for s in (2, 3):
                for pad in (0, 3):
                    run_gemm_bf16_tn(r, R, G, s, ldc_pad=pad, ws_bytes=ws(M, N, s), check='bf16 tn %d slices ldc N + %d' % (s, pad))
            run_gemm_bf16_tn(r, R, G, 2, lda_pad=64, ws_bytes=ws(M, N, 2), check='bf16 tn lda + 64')
            run_gemm_bf16_tn(r, R, G[:, :32], 2, ldc_pad=8, ws_bytes=ws(M, 32, 2), check='bf16 tn 129 x 32 ldc N + 8')
        else:
            transposed = int(op[-1])
            N, rows, cols = 33, 129, 201
            Rb = (rs.rand(rows, cols) < 0.3).astype(np.float64)
            G = rs.randn(rows if transposed else cols, N)
            M = cols if transposed else rows
            for pad in (0, 3):
                run_gemm_bits(r, Rb, G, transposed, 2, ldc_pad=pad, ws_bytes=ws(M, N, 2), check='bf16 %s ldc N + %d' % (op, pad))
    assert g.bands > 0


def test_workspaces_are_exact(rt):
    """skf_pinv_sym, skf_fill_unknown and the three completion operators (col_splits 0 and 3; top-k also 2, where the last
    of its partial lists is written, and k = 64, where a list is as long as the granule of the sizes) on exactly the bytes their
    query returns, between guard bands; one byte fewer: SKF_E_WORKSPACE and outputs untouched (the completion operators'
    refusals: their own cases, under guard)."""
    import complete_cases as CC
    import ranks_cases as RC
    import above_cases as AC
    from guarded import guarded
    rs = np.random.RandomState(14)
    with guarded(rt) as g:
        r, mem = g.rt, g.rt.mem
        for n in (33, 70):
            G = rs.rand(3 * n, n)
            A = G.T @ G
            assert relerr(A @ run_pinv(r, nat.SKF_F64, A) @ A, A) < 1e-11          # (run_pinv: exactly the queried bytes)
            need = C.c_size_t()
            r.call('skf_pinv_sym_workspace_bytes', n, C.byref(need))
            a, k, ws = mem.from_host(A), mem.from_host(np.full((n, n), -7.0)), mem.empty(need.value)
            rc = r.lib.skf_pinv_sym(nat.SKF_F64, a.ptr, n, k.ptr, n, n, ws.ptr, need.value - 1, None)
            mem.synchronize()
            assert rc == nat.SKF_E_WORKSPACE and (mem.to_host(k, (n, n), np.float64) == -7.0).all()
        rows, cols = 37, 53
        X = rs.rand(rows, cols)
        X[rs.rand(rows, cols) < 0.2] = np.nan
        need = C.c_size_t()
        r.call('skf_fill_unknown_workspace_bytes', rows, cols, C.byref(need))
        for strategy, want in ((0, np.where(np.isnan(X), np.nanmean(X), X)),
                               (1, np.where(np.isnan(X), np.nanmean(X, axis=1)[:, None], X)),
                               (2, np.where(np.isnan(X), np.nanmean(X, axis=0)[None, :], X))):
            x, ws = mem.from_host(X), mem.empty(need.value)
            rc = r.lib.skf_fill_unknown(nat.SKF_F64, x.ptr, cols, rows, cols, None, 0, strategy, 0.0, ws.ptr, need.value - 1, None)
            mem.synchronize()
            assert rc == nat.SKF_E_WORKSPACE
            np.testing.assert_array_equal(mem.to_host(x, (rows, cols), np.float64), X)
            r.call('skf_fill_unknown', nat.SKF_F64, x.ptr, cols, rows, cols, None, 0, strategy, 0.0, ws.ptr, need.value, None)
            mem.synchronize()
            np.testing.assert_allclose(mem.to_host(x, (rows, cols), np.float64), want, rtol=1e-13, atol=0)
        for dtype in ('f64', 'f32'):
            CC.exact_case(dtype, 67, 203, (5, 7), ks=(10, 64), patterns=('edges',), splits=(0, 2, 3))
            RC.exact_case(dtype, 67, 203, (5, 7), patterns=('edges',), splits=(0, 3))
            AC.exact_case(dtype, 67, 203, (5, 7), patterns=('edges',), splits=(0, 3))
            CC.refusals_case(dtype)
            RC.refusals_case(dtype)
            AC.refusals_case(dtype)
    assert g.bands > 0
