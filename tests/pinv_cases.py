"""Shared cases of the pseudo-inverse (csrc/skf_pinv.h, skf_pinv.inc) for the emulator tests, their GPU twins and
tools/ab_pinv.py: the stand-alone operator on matrices whose leading dimensions exceed the order, and a plan of 17 types --
one more than a pack / unpack launch holds (PINV_MAXB = 16)."""
import ctypes as C

import numpy as np

import skfusion_amd._native as nat

POISON = 0xA5
PINV_MAXB = 16


def dyadic(rs, rows, cols):
    """Entries k / 8, k = 1 .. 8: the Gram matrix of up to 2^18 such rows is exact in f32 as well as in f64, so the f32 cases
    see the matrix the f64 cases see and scipy's f64 result is the reference of both."""
    return np.floor(rs.rand(rows, cols) * 8.0 + 1.0) / 8.0


def strided_matrix(n, rank=None):
    """Gram matrix of order n: full rank (4 n + 3 rows, as test_pinv_full_rank_matches_scipy) or of `rank` rows with an exactly
    duplicated latent column (as test_pinv_deflation_matches_scipy_and_the_eigen_path)."""
    rs = np.random.RandomState(1000 * n + (rank or 0))
    if rank is None:
        G = dyadic(rs, 4 * n + 3, n)
    else:
        G = dyadic(rs, rank, n)
        G[:, n // 2] = G[:, 1]
    return G.T @ G


def run_pinv_strided(rt, dtype, A, lda, ldk):
    """skf_pinv_sym on A stored with leading dimension lda, into a K of leading dimension ldk filled with poison bytes.
    Returns K[:, :n], the bytes of columns n .. ldk - 1 after the call, the verdict word (1: an inverse written straight into
    K; 2: the one-workgroup deflation; 0: the eigen-solver) and the launches of the call."""
    from skfusion_amd._engine import launch_count
    npd = nat.NP_DTYPE[dtype]
    n = A.shape[0]
    need = C.c_size_t()
    rt.call('skf_pinv_sym_workspace_bytes', n, C.byref(need))
    Ain = np.full((n, lda), np.nan, npd)
    Ain[:, :n] = A
    a = rt.mem.from_host(Ain)
    k = rt.mem.from_host(np.full(n * ldk * np.dtype(npd).itemsize, POISON, np.uint8))
    ws = rt.mem.empty(need.value)
    before = launch_count(rt)
    rt.call('skf_pinv_sym', dtype, a.ptr, lda, k.ptr, ldk, n, ws.ptr, need.value, None)
    launches = launch_count(rt) - before
    npad = (n + 1) // 2 * 2
    mat = (npad * npad * 8 + 255) // 256 * 256
    off = 3 * mat + (npad * 8 + 255) // 256 * 256 + 32 * 4
    verdict = int(rt.mem.to_host(ws, (need.value // 4,), np.int32)[off // 4])
    got = rt.mem.to_host(k, (n, ldk), npd)
    return got[:, :n].copy(), np.ascontiguousarray(got[:, n:]).view(np.uint8), verdict, launches


def chain17_graph():
    """A chain t0 - t1 - ... - t16: 12 .. 40 objects and ranks 3 .. 8 per type; the last type has 6 objects and rank 8, so its
    Gram matrix is rank-deficient by construction and the fast path declines it in every iteration -- in the SECOND chunk of
    the pack / unpack launches, whose base and verdict pointers are offset by 16 matrices."""
    rs = np.random.RandomState(17)
    types = ['t%d' % k for k in range(PINV_MAXB + 1)]
    n = {t: 12 + (11 * k) % 29 for k, t in enumerate(types)}
    rank = {t: 3 + k % 6 for k, t in enumerate(types)}
    n[types[-1]], rank[types[-1]] = 6, 8
    R = {(a, b): [rs.rand(n[a], n[b])] for a, b in zip(types[:-1], types[1:])}
    G0 = {(t, t): rs.rand(n[t], rank[t]) + 0.05 for t in types}
    return R, types, rank, G0
