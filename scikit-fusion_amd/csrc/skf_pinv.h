// skf_pinv.h -- kernels of the pseudo-inverse K = pinv(Gram) of a symmetric positive semi-definite matrix, f64 throughout
// (host side: skf_pinv.inc; the small-graph schedule calls the device bodies from skf_small.h).
//
// Kernels, in the order of the route cascade
//   eigh_pack_kernel<T>            the caller's matrices -> the f64 eigen workspace, padded to an even order
//   chol_inverse*_kernel           Cholesky fast path (one wave / LDS-blocked / plain) with an on-device verdict
//   sweep_inverse_kernel,          blocked sweep operator, orders 65 .. SWEEP_MAXN in one launch / up to EIGH_MAXN one launch
//   sweep_step_kernel<BIG>         per block step: writes K itself
//   chol_unpack_kernel<T>          K = X^T X from the inverted Cholesky factor
//   pchol_*_kernel                 rank-revealing deflation over several workgroups (orders above SWEEP_MAXN)
//   pchol_pinv_kernel              ... in one workgroup
//   jacobi_eigh_kernel             symmetric eigen-decomposition (parallel two-sided cyclic Jacobi, one workgroup per
//                                  matrix) -> pinv with the SVD cut-off of scipy.linalg.pinv (reference _dfmf.py:232)
//   eigh_unpack_pinv_kernel<T>     K = Vs V^T for the matrices the deflation / the eigen-solver produced
#pragma once
#include "skf_kernels.h"

namespace skf {

// ------------------------------------------------------------------------------------------
// Symmetric eigen-decomposition by parallel two-sided cyclic Jacobi (f64), one workgroup per
// matrix (blockIdx.x selects the matrix).  A (n x n, row-major, ld = n) is overwritten; V
// receives the eigenvectors as columns; w the eigenvalues.  n must be even (the host pads an
// odd matrix with one decoupled row/column).  Round-robin ("chess tournament") ordering gives
// n/2 disjoint rotation pairs per round and n-1 rounds per sweep.
// Afterwards:  Vs = V * diag(winv),  winv_k = 1/w_k if |w_k| > n_orig * eps * max|w| else 0
// (scipy.linalg.pinv cut-off, rtol = max(M,N)*eps), so that pinv(A) = Vs * V^T.
// ------------------------------------------------------------------------------------------
struct EighArgs {
    double* A;        // [batch] pointers are derived as A + b*stride
    double* V;
    double* Vs;
    double* w;
    int64_t stride;   // elements between consecutive matrices in A / V / Vs
    int64_t wstride;
    const int* n;     // per-matrix (padded, even) order
    const int* n_orig;
    int* chol_ok;     // per matrix: 1 = the Cholesky fast path produced the inverse, 2 = the rank-revealing deflation
                      // did (result in the eigen format Vs, V); 0 = left to the Jacobi eigen-solver
    int max_sweeps;
};

constexpr int EIGH_THREADS = 512;
constexpr int EIGH_MAXN = 1024;

__device__ __forceinline__ void jacobi_pair(int round, int k, int n, int& p, int& q) {
    // players 0..n-1, player n-1 fixed, the others rotate
    const int m = n - 1;
    int a, b;
    if (k == 0) {
        a = n - 1;
        b = round % m;
    } else {
        a = (round + k) % m;
        b = (round - k + m) % m;
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

__device__ __forceinline__ void jacobi_eigh_body(const EighArgs& e, const int b) {
    __shared__ double cs[EIGH_MAXN / 2], sn[EIGH_MAXN / 2];
    __shared__ int pp[EIGH_MAXN / 2], qq[EIGH_MAXN / 2];
    __shared__ double red[EIGH_THREADS / 64];
    __shared__ double s_off, s_diag;
    __shared__ int s_rot;                     // some pair rotated in the current sweep
    if (e.chol_ok[b]) return;                 // uniform: fast path already inverted this matrix
    const int n = e.n[b];
    const int tid = threadIdx.x, nt = blockDim.x;
    double* A = e.A + (int64_t)b * e.stride;
    double* V = e.V + (int64_t)b * e.stride;
    double* Vs = e.Vs + (int64_t)b * e.stride;
    double* w = e.w + (int64_t)b * e.wstride;
    const int half = n / 2;

    // symmetrise, V = I
    for (int idx = tid; idx < n * n; idx += nt) {
        const int r = idx / n, c = idx % n;
        V[idx] = (r == c) ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += nt) {
        const int r = idx / n, c = idx % n;
        if (r < c) {
            const double s = 0.5 * (A[r * n + c] + A[c * n + r]);
            A[r * n + c] = s;
            A[c * n + r] = s;
        }
    }
    __syncthreads();

    for (int sweep = 0; sweep < e.max_sweeps; ++sweep) {
        // convergence: off-diagonal Frobenius mass relative to the diagonal
        double off = 0.0, dg = 0.0;
        for (int idx = tid; idx < n * n; idx += nt) {
            const int r = idx / n, c = idx % n;
            const double v = A[idx];
            if (r == c) dg += v * v; else off += v * v;
        }
        off = wave_sum(off);
        dg = wave_sum(dg);
        if ((tid & 63) == 0) red[tid >> 6] = off;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int i = 0; i < nt / 64; ++i) s += red[i];
            s_off = s;
        }
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = dg;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int i = 0; i < nt / 64; ++i) s += red[i];
            s_diag = s;
            s_rot = 0;
        }
        __syncthreads();
        if (s_off <= 1e-30 * s_diag || s_off == 0.0) break;       // uniform across the block
        const double s_dnorm = sqrt(s_diag);

        for (int round = 0; round < n - 1; ++round) {
            // phase 1: rotation angles of the n/2 disjoint pairs
            for (int k = tid; k < half; k += nt) {
                int p, q;
                jacobi_pair(round, k, n, p, q);
                const double app = A[p * n + p], aqq = A[q * n + q], apq = A[p * n + q];
                double c = 1.0, s = 0.0;
                // threshold Jacobi: an off-diagonal entry below 1e-2 * eps of the diagonal's norm is left
                // alone.  That is 100x under the absolute accuracy eps * ||A|| of the LAPACK SVD behind
                // scipy.linalg.pinv and far under the cut-off n * eps * sigma_max; it is what lets a
                // rank-deficient Gram matrix converge: its null-space block consists of rounding noise
                // at eps * ||A|| that cyclic rotations never bring to exactly zero (30 sweeps before,
                // now the usual 8-10).  Pairs that do not rotate move no data.
                if (apq != 0.0 && fabs(apq) > 2.2e-18 * s_dnorm) {
                    const double tau = (aqq - app) / (2.0 * apq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                    if (s != 0.0) s_rot = 1;      // benign race: every writer stores 1
                }
                cs[k] = c; sn[k] = s; pp[k] = p; qq[k] = q;
            }
            __syncthreads();
            // phase 2: columns  A <- A J,  V <- V J   (row r, pair k)
            for (int idx = tid; idx < n * half; idx += nt) {
                const int r = idx / half, k = idx % half;
                const int p = pp[k], q = qq[k];
                const double c = cs[k], s = sn[k];
                if (s == 0.0) continue;
                const double arp = A[r * n + p], arq = A[r * n + q];
                A[r * n + p] = c * arp - s * arq;
                A[r * n + q] = s * arp + c * arq;
                const double vrp = V[r * n + p], vrq = V[r * n + q];
                V[r * n + p] = c * vrp - s * vrq;
                V[r * n + q] = s * vrp + c * vrq;
            }
            __syncthreads();
            // phase 3: rows  A <- J^T A   (pair k, column col)
            for (int idx = tid; idx < half * n; idx += nt) {
                const int k = idx / n, col = idx % n;
                const int p = pp[k], q = qq[k];
                const double c = cs[k], s = sn[k];
                if (s == 0.0) continue;
                const double apc = A[p * n + col], aqc = A[q * n + col];
                A[p * n + col] = c * apc - s * aqc;
                A[q * n + col] = s * apc + c * aqc;
            }
            __syncthreads();
        }
        if (!s_rot) break;                       // a whole sweep without a rotation: converged (uniform)
    }

    // eigenvalues, cut-off, scaled eigenvectors
    double mx = 0.0;
    for (int k = tid; k < n; k += nt) {
        const double v = A[k * n + k];
        w[k] = v;
        mx = fmax(mx, fabs(v));
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < nt / 64; ++i) s = fmax(s, red[i]);
        s_off = s;
    }
    __syncthreads();
    const double thr = (double)e.n_orig[b] * 2.220446049250313e-16 * s_off;
    for (int idx = tid; idx < n * n; idx += nt) {
        const int c = idx % n;
        const double wc = w[c];
        const double inv = (fabs(wc) > thr) ? 1.0 / wc : 0.0;
        Vs[idx] = V[idx] * inv;
    }
}
static __global__ __launch_bounds__(EIGH_THREADS) void jacobi_eigh_kernel(EighArgs e) { jacobi_eigh_body(e, blockIdx.x); }

// ------------------------------------------------------------------------------------------
// Fast path of the pseudo-inverse: a symmetric positive definite Gram matrix whose pivots stay
// above rel_thr * max(diag) is inverted through its Cholesky factor (pinv == inverse when no
// singular value falls under the cut-off).  One workgroup per matrix:
//   L L^T = A   right-looking, column k staged in LDS, 2 barriers per column
//   X = L^-1    one thread per column (forward substitution)
// and chol_unpack_kernel forms K = X^T X on the whole grid.  A failed pivot test sets
// chol_ok[b] = 0 and leaves the matrix to the Jacobi eigen-solver above (rank-deficient /
// severely ill-conditioned Gram matrices, reference tests/test_n_run.py:14).
// Scratch: L lives in e.Vs, X in e.V (both are only written by the Jacobi path afterwards).
// ------------------------------------------------------------------------------------------
// Pivot test of the fast path.  Cholesky is invariant under diagonal scaling, so a pivot is judged
// against ITS OWN diagonal entry: p_k / a_kk = sin^2 of the angle between factor column k and the span
// of the columns before it -- below rel_thr the columns are (nearly) dependent and the exact
// pseudo-inverse semantics of the eigen path are needed.  A mere difference in scale between the
// columns (a latent dimension 1e-5 times smaller than the largest) stays on the fast path; only
// a diagonal entry so small that scipy.linalg.pinv's cut-off (n * eps * sigma_max, sigma_max <= n *
// max diag) could truncate its direction is handed to the eigen path.
__device__ __forceinline__ double chol_diag_floor(int n) { return (double)n * (double)n * 2.220446049250313e-16; }

static __global__ __launch_bounds__(EIGH_THREADS) void chol_inverse_kernel(EighArgs e, double rel_thr) {
    __shared__ double col[EIGH_MAXN];
    __shared__ double red[EIGH_THREADS / 64];
    __shared__ double s_max;
    const int b = blockIdx.x;
    const int n = e.n_orig[b], ld = e.n[b];
    const int tid = threadIdx.x, nt = blockDim.x;
    const double* A = e.A + (int64_t)b * e.stride;
    double* L = e.Vs + (int64_t)b * e.stride;
    double* X = e.V + (int64_t)b * e.stride;

    double mx = 0.0;
    for (int idx = tid; idx < n * n; idx += nt) {
        const int r = idx / n, c = idx % n;
        const double v = 0.5 * (A[r * ld + c] + A[c * ld + r]);
        L[r * ld + c] = v;
        X[r * ld + c] = 0.0;
        if (r == c) mx = fmax(mx, fabs(v));
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < nt / 64; ++i) s = fmax(s, red[i]);
        s_max = s;
    }
    __syncthreads();
    const double floor_ = chol_diag_floor(n) * s_max;

    for (int k = 0; k < n; ++k) {
        const double piv = L[k * ld + k];
        const double akk = A[k * ld + k];
        if (!(akk > floor_) || !(piv > rel_thr * akk) || !(piv > 0.0)) {   // uniform: every thread reads the same words
            if (tid == 0) e.chol_ok[b] = 0;
            return;
        }
        const double d = sqrt(piv);
        for (int i = k + tid; i < n; i += nt) col[i] = (i == k) ? d : L[i * ld + k] / d;
        __syncthreads();
        // write the finished column and update the trailing lower triangle
        const int m = n - k - 1;
        for (int i = k + tid; i < n; i += nt) L[i * ld + k] = col[i];
        for (int idx = tid; idx < m * m; idx += nt) {
            const int i = k + 1 + idx / m, j = k + 1 + idx % m;
            if (j <= i) L[i * ld + j] -= col[i] * col[j];
        }
        __syncthreads();
    }
    // X = L^-1 by forward substitution of L X = I: thread j owns column j and never reads another
    // thread's data, so no barrier is needed.  The loops run over uniform bounds (q < i for every
    // lane; the structurally zero X(q,j), q < j, are simply multiplied in): L(i,q) is then a
    // wave-uniform (scalar) load and the X column loads are coalesced and pipeline freely.
    __syncthreads();
    for (int j = tid; j < n; j += nt) {
        for (int i = 0; i < n; ++i) {
            const double* Li = L + i * ld;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int q = 0;
            for (; q + 3 < i; q += 4) {
                s0 += Li[q] * X[q * ld + j];
                s1 += Li[q + 1] * X[(q + 1) * ld + j];
                s2 += Li[q + 2] * X[(q + 2) * ld + j];
                s3 += Li[q + 3] * X[(q + 3) * ld + j];
            }
            for (; q < i; ++q) s0 += Li[q] * X[q * ld + j];
            const double rhs = (i == j) ? 1.0 : 0.0;
            X[i * ld + j] = (rhs - ((s0 + s1) + (s2 + s3))) / Li[i];
        }
    }
    if (tid == 0) e.chol_ok[b] = 1;
}

// ------------------------------------------------------------------------------------------
// Small orders (n <= 64: the ranks of the reference's own examples): one 64-lane workgroup per
// matrix, everything in LDS, lane i owns row i of L and column i of X = L^-1 (stored transposed,
// so both are bank-conflict-free private rows of pitch 65).  Same contract as chol_inverse_kernel
// (X in e.V, verdict in chol_ok); ~10 us instead of ~100 us for the blocked kernel on a 50 x 50
// matrix -- on small graphs the pseudo-inverse chain is the critical path of an iteration.
// ------------------------------------------------------------------------------------------
constexpr int CHOLS_MAXN = 64;

static __global__ __launch_bounds__(64) void chol_inverse_small_kernel(EighArgs e, double rel_thr) {
    constexpr int LD = CHOLS_MAXN + 1;
    // one array: L in the lower triangle and on the diagonal, X^T strictly above it
    // (M[j][r] = X(r, j) for r > j; X(j, j) = 1 / L(j, j) is not stored)
    __shared__ double M[CHOLS_MAXN * LD];
    __shared__ double col[CHOLS_MAXN];
    const int b = blockIdx.x;
    const int n = e.n_orig[b], ld = e.n[b];
    const int i = threadIdx.x;
    const double* A = e.A + (int64_t)b * e.stride;
    double* X = e.V + (int64_t)b * e.stride;

    double mx = 0.0;
    if (i < n) {
        for (int c = 0; c <= i; ++c) M[i * LD + c] = 0.5 * (A[i * ld + c] + A[c * ld + i]);
        mx = fabs(M[i * LD + i]);
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    const double floor_ = chol_diag_floor(n) * mx;
    __syncthreads();

    for (int k = 0; k < n; ++k) {
        const double piv = M[k * LD + k];
        const double akk = A[k * ld + k];
        if (!(akk > floor_) || !(piv > rel_thr * akk) || !(piv > 0.0)) {   // uniform
            if (i == 0) e.chol_ok[b] = 0;
            return;
        }
        const double d = sqrt(piv);
        double lik = 0.0;
        if (i >= k && i < n) {
            lik = (i == k) ? d : M[i * LD + k] / d;
            col[i] = lik;
        }
        __syncthreads();
        if (i >= k && i < n) {
            M[i * LD + k] = lik;
            for (int j = k + 1; j <= i; ++j) M[i * LD + j] -= lik * col[j];
        }
        __syncthreads();
    }
    // X = L^-1: lane j solves L x = e_j (column j of X, kept as row j above the diagonal); the L rows
    // are wave-uniform broadcasts, the x entries lane-private
    if (i < n) {
        const int j = i;
        const double xjj = 1.0 / M[j * LD + j];
        for (int r = j + 1; r < n; ++r) {
            double s = M[r * LD + j] * xjj;
            for (int q = j + 1; q < r; ++q) s += M[r * LD + q] * M[j * LD + q];
            M[j * LD + r] = -s / M[r * LD + r];
        }
    }
    __syncthreads();
    if (i < n)
        for (int c = 0; c < n; ++c)
            X[i * ld + c] = (c < i) ? M[c * LD + i] : (c == i ? 1.0 / M[i * LD + i] : 0.0);
    if (i == 0) e.chol_ok[b] = 1;
}

// ------------------------------------------------------------------------------------------
// LDS-blocked version of the fast path (orders up to CHOLB_MAXN): the same contract as
// chol_inverse_kernel -- L in e.Vs, X = L^-1 in e.V, verdict in chol_ok -- with NB = 32 column
// panels.  Per panel: the diagonal block is factored in LDS, the rows below are solved one per
// thread against it and kept as a transposed panel in LDS, and the trailing matrix receives one
// rank-32 update (global memory is touched once per panel instead of once per column).
// X = L^-1 by block forward substitution: the diagonal blocks are inverted first, then wave w
// walks down block column w with 32x32x32 register-tiled products.
// Dynamic LDS: D[32][33] + max(P[32][n], 8 waves x T[32][33]) doubles.
// ------------------------------------------------------------------------------------------
constexpr int CHOLB_NB = 32;
constexpr int CHOLB_MAXN = 512;

static __global__ __launch_bounds__(EIGH_THREADS) void chol_inverse_blocked_kernel(EighArgs e, double rel_thr) {
    constexpr int NB = CHOLB_NB;
    HIP_DYNAMIC_SHARED(double, csm)
    __shared__ double red[EIGH_THREADS / 64];
    __shared__ double s_max;
    const int b = blockIdx.x;
    const int n = e.n_orig[b], ld = e.n[b];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = nt >> 6;
    const double* A = e.A + (int64_t)b * e.stride;
    double* L = e.Vs + (int64_t)b * e.stride;
    double* X = e.V + (int64_t)b * e.stride;
    double* D = csm;                       // [NB][NB+1]
    double* P = csm + NB * (NB + 1);       // [NB][n]  transposed panel  /  per-wave T tiles later

    double mx = 0.0;
    for (int idx = tid; idx < n * n; idx += nt) {
        const int r = idx / n, c = idx % n;
        const double v = 0.5 * (A[r * ld + c] + A[c * ld + r]);
        L[r * ld + c] = v;
        X[r * ld + c] = 0.0;
        if (r == c) mx = fmax(mx, fabs(v));
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < nwaves; ++i) s = fmax(s, red[i]);
        s_max = s;
    }
    __syncthreads();
    const double floor_ = chol_diag_floor(n) * s_max;

    // ---------------- factorisation
    for (int kb = 0; kb < n; kb += NB) {
        const int nb = (n - kb < NB) ? n - kb : NB;
        const int m = n - kb - nb;                       // rows below the diagonal block
        for (int idx = tid; idx < nb * nb; idx += nt) {
            const int r = idx / nb, c = idx % nb;
            D[r * (NB + 1) + c] = L[(kb + r) * ld + kb + c];
        }
        __syncthreads();
        for (int k = 0; k < nb; ++k) {
            const double piv = D[k * (NB + 1) + k];
            const double akk = A[(kb + k) * ld + kb + k];
            if (!(akk > floor_) || !(piv > rel_thr * akk) || !(piv > 0.0)) {   // uniform: same words for every thread
                if (tid == 0) e.chol_ok[b] = 0;
                return;
            }
            const double d = sqrt(piv);
            __syncthreads();                              // everybody has read the pivot
            for (int r = k + tid; r < nb; r += nt) D[r * (NB + 1) + k] = (r == k) ? d : D[r * (NB + 1) + k] / d;
            __syncthreads();
            const int w = nb - k - 1;
            for (int idx = tid; idx < w * w; idx += nt) {
                const int r = k + 1 + idx / w, c = k + 1 + idx % w;
                if (c <= r) D[r * (NB + 1) + c] -= D[r * (NB + 1) + k] * D[c * (NB + 1) + k];
            }
            __syncthreads();
        }
        // diagonal block back to global; panel rows: x = a * L11^-T, one row per thread
        for (int idx = tid; idx < nb * nb; idx += nt) {
            const int r = idx / nb, c = idx % nb;
            if (c <= r) L[(kb + r) * ld + kb + c] = D[r * (NB + 1) + c];
        }
        for (int i = tid; i < m; i += nt) {
            double* row = L + (int64_t)(kb + nb + i) * ld + kb;
            double x[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) x[c] = (c < nb) ? row[c] : 0.0;
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                if (c < nb) {
                    double s = x[c];
#pragma unroll
                    for (int q = 0; q < NB; ++q)
                        if (q < c) s -= x[q] * D[c * (NB + 1) + q];
                    x[c] = s / D[c * (NB + 1) + c];
                }
            }
#pragma unroll
            for (int c = 0; c < NB; ++c)
                if (c < nb) {
                    row[c] = x[c];
                    P[c * n + i] = x[c];
                }
        }
        __syncthreads();
        // trailing update of the lower triangle: L22 -= L21 L21^T
        for (int idx = tid; idx < m * m; idx += nt) {
            const int i = idx / m, j = idx % m;
            if (j <= i) {
                double s = 0.0;
#pragma unroll 8
                for (int c = 0; c < nb; ++c) s += P[c * n + i] * P[c * n + j];
                L[(int64_t)(kb + nb + i) * ld + kb + nb + j] -= s;
            }
        }
        __syncthreads();
    }

    // ---------------- X = L^-1
    const int nblk = (n + NB - 1) / NB;
    // (a) inverses of the diagonal blocks: 32 threads per block, one column each
    for (int t = tid; t < nblk * NB; t += nt) {
        const int blk = t / NB, j = t % NB;
        const int b0 = blk * NB;
        const int nb = (n - b0 < NB) ? n - b0 : NB;
        if (j < nb) {
            double x[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                x[i] = 0.0;
                if (i < nb && i >= j) {
                    double s = (i == j) ? 1.0 : 0.0;
#pragma unroll
                    for (int q = 0; q < NB; ++q)
                        if (q < i && q >= j) s -= L[(int64_t)(b0 + i) * ld + b0 + q] * x[q];
                    x[i] = s / L[(int64_t)(b0 + i) * ld + b0 + i];
                }
            }
#pragma unroll
            for (int i = 0; i < NB; ++i)
                if (i < nb && i >= j) X[(int64_t)(b0 + i) * ld + b0 + j] = x[i];
        }
    }
    __syncthreads();
    // (b) block forward substitution: X[ib,jb] = -Xd[ib] * sum_{kb=jb}^{ib-1} L[ib,kb] X[kb,jb]
    double* T = P + wave * NB * (NB + 1);                 // per-wave 32 x 33 tile
    const int r0 = 4 * (lane >> 3), c0 = 4 * (lane & 7);  // 4 x 4 outputs per lane
    for (int ib = 1; ib < nblk; ++ib) {
        const int i0 = ib * NB;
        for (int jb = wave; jb < ib; jb += nwaves) {
            const int j0 = jb * NB;
            double acc[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
            for (int k = j0; k < i0; ++k) {               // k runs over the columns of L[ib, jb..ib-1]
                double a[4], bb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] = (i0 + r0 + u < n) ? L[(int64_t)(i0 + r0 + u) * ld + k] : 0.0;
#pragma unroll
                for (int v = 0; v < 4; ++v) bb[v] = X[(int64_t)k * ld + j0 + c0 + v];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] += a[u] * bb[v];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) T[(r0 + u) * (NB + 1) + c0 + v] = acc[u][v];
            // the tile is produced and consumed by the same wave: order the LDS traffic
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = r0 + u;
                double o[4] = {0.0, 0.0, 0.0, 0.0};
                if (i0 + r < n) {
                    for (int q = 0; q <= r; ++q) {
                        const double dv = X[(int64_t)(i0 + r) * ld + i0 + q];
#pragma unroll
                        for (int v = 0; v < 4; ++v) o[v] += dv * T[q * (NB + 1) + c0 + v];
                    }
#pragma unroll
                    for (int v = 0; v < 4; ++v) X[(int64_t)(i0 + r) * ld + j0 + c0 + v] = -o[v];
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
    }
    if (tid == 0) e.chol_ok[b] = 1;
}

// ------------------------------------------------------------------------------------------
// Rank-revealing deflation: the pseudo-inverse of a symmetric positive SEMI-definite matrix the Cholesky fast
// path rejected (a rank-deficient Gram matrix: duplicate or zero latent columns, rank > objects -- the case of
// reference tests/test_n_run.py:14), without an eigen-decomposition:
//   1. Cholesky with complete diagonal pivoting, stopped when the largest remaining diagonal entry falls below
//      lo * d_max:   A = L L^T + (remainder <= n * lo * d_max),  L: n x r, r = numerical rank
//   2. A^+ = Y Y^T with Y = L (L^T L)^-1  (exact for a matrix of rank r): B = L^T L (r x r, positive definite),
//      its Cholesky factor, and one forward + backward substitution per row of L.
// scipy.linalg.pinv (reference _dfmf.py:232) cuts singular values <= n * eps * sigma_max instead.  The two agree
// to rounding when the spectrum has a GAP between the kept part and rounding noise, which the kernel checks on
// the pivots it is given: no accepted pivot below hi * d_max (lo = 1e-10, hi = 1e-7 relative to the largest
// diagonal entry).  A pivot inside (lo, hi) * d_max -- a genuinely ill-conditioned matrix -- leaves chol_ok = 0 and
// the Jacobi eigen-solver applies the exact cut-off.  One workgroup per matrix; 1.1 ms instead of 216 ms for a
// rank-128 matrix of order 256 (tools/bench_pinv.py).  Result in the eigen format: Vs = V = Y (row-major, zero
// padded), so that eigh_unpack_pinv forms K = Vs V^T.
// ------------------------------------------------------------------------------------------
constexpr int PCHOL_LDS_R = 176;           // packed r (r + 1) / 2 doubles of the small factor fit the dynamic LDS up to this rank
constexpr int PCHOL_LDS_BYTES = PCHOL_LDS_R * (PCHOL_LDS_R + 1) / 2 * 8;
__device__ __forceinline__ void pchol_pinv_body(const EighArgs& e, const int b, double lo, double hi, int lds_rank) {
    __shared__ double d[EIGH_MAXN];            // remaining diagonal; < 0: the index has been a pivot
    __shared__ double rowk[EIGH_MAXN];         // row of L of the current pivot (its first k entries)
    __shared__ double red_v[EIGH_THREADS / 64];
    __shared__ int red_i[EIGH_THREADS / 64];
    __shared__ double s_val;
    __shared__ int s_idx, s_fail;
    if (e.chol_ok[b] || !(lo < 1.0)) return;   // uniform: the fast path inverted this matrix / deflation switched off
    const int n = e.n[b];
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const double* A = e.A + (int64_t)b * e.stride;
    double* Lt = e.V + (int64_t)b * e.stride;      // Lt[k * n + i] = L[i][k]   (column k contiguous over the rows)
    double* W = e.Vs + (int64_t)b * e.stride;      // B = L^T L, then its Cholesky factor (r x r, row-major, ld n)

    for (int i = tid; i < n; i += nt) d[i] = A[(int64_t)i * n + i];
    if (tid == 0) s_fail = 0;
    __syncthreads();
    double dmax0 = 0.0, last = 0.0;
    int r = 0;
    for (int k = 0; k < n; ++k) {
        // ---- pivot = the largest remaining diagonal entry
        double bv = -1.0;
        int bi = -1;
        for (int i = tid; i < n; i += nt)
            if (d[i] > bv) { bv = d[i]; bi = i; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi >= 0 && (bi < 0 || oi < bi))) { bv = ov; bi = oi; }
        }
        if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            double v = red_v[0];
            int ix = red_i[0];
            for (int w = 1; w < nt / 64; ++w)
                if (red_v[w] > v || (red_v[w] == v && red_i[w] >= 0 && (ix < 0 || red_i[w] < ix))) { v = red_v[w]; ix = red_i[w]; }
            s_val = v;
            s_idx = ix;
        }
        __syncthreads();
        const double pv = s_val;
        const int piv = s_idx;
        if (k == 0) dmax0 = pv;
        if (piv < 0 || !(pv > lo * dmax0) || !(pv > 0.0)) break;          // uniform: everything left is noise
        last = pv;
        r = k + 1;
        const double lkk = sqrt(pv);
        for (int j = tid; j < k; j += nt) rowk[j] = Lt[(int64_t)j * n + piv];
        __syncthreads();
        for (int i = tid; i < n; i += nt) {
            double v;
            if (i == piv) {
                v = lkk;
            } else if (d[i] < 0.0) {
                v = 0.0;                                                   // an earlier pivot: above the diagonal
            } else {
                double sacc = A[(int64_t)i * n + piv];
                for (int j = 0; j < k; ++j) sacc -= Lt[(int64_t)j * n + i] * rowk[j];
                v = sacc / lkk;
                const double nd = d[i] - v * v;
                d[i] = nd > 0.0 ? nd : 0.0;
            }
            Lt[(int64_t)k * n + i] = v;
        }
        __syncthreads();
        if (tid == 0) d[piv] = -1.0;
        __syncthreads();
    }
    if (r > 0 && last < hi * dmax0) return;    // uniform: a pivot in the ambiguous band -> exact cut-off (Jacobi)

    // ---- B = L^T L (r x r, lower triangle, packed: element (a, c <= a) at a (a + 1) / 2 + c) -- in LDS when it fits
    // (r <= PCHOL_LDS_R), else in the Vs scratch.  One wave per element: the lanes split the rows (coalesced) and meet
    // in a wave reduction.
    HIP_DYNAMIC_SHARED(double, Cs)
    const bool in_lds = r <= lds_rank;          // the launch reserved lds_rank (lds_rank + 1) / 2 doubles of dynamic LDS
    double* Cp = in_lds ? Cs : W;
    const int nel = r * (r + 1) / 2;
    for (int el = wave; el < nel; el += nt / 64) {
        int a = (int)((sqrt(8.0 * el + 1.0) - 1.0) * 0.5);
        while ((a + 1) * (a + 2) / 2 <= el) ++a;
        while (a * (a + 1) / 2 > el) --a;
        const int c = el - a * (a + 1) / 2;
        double sacc = 0.0;
        for (int i = lane; i < n; i += 64) sacc += Lt[(int64_t)a * n + i] * Lt[(int64_t)c * n + i];
        sacc = wave_sum(sacc);
        if (lane == 0) Cp[el] = sacc;
    }
    __syncthreads();
    // ---- Cholesky of B in place, right-looking
    for (int k = 0; k < r; ++k) {
        const int kk = k * (k + 1) / 2;
        const double pk = Cp[kk + k];
        if (!(pk > 0.0)) {
            if (tid == 0) s_fail = 1;
        }
        __syncthreads();
        if (s_fail) return;                    // uniform (A is untouched: the eigen-solver takes over)
        const double ck = sqrt(pk);
        for (int i = k + 1 + tid; i < r; i += nt) Cp[i * (i + 1) / 2 + k] /= ck;
        __syncthreads();
        if (tid == 0) Cp[kk + k] = ck;
        const int m = r - k - 1;
        for (int idx = tid; idx < m * m; idx += nt) {
            const int i = k + 1 + idx / m, j = k + 1 + idx % m;
            if (j <= i) Cp[i * (i + 1) / 2 + j] -= Cp[i * (i + 1) / 2 + k] * Cp[j * (j + 1) / 2 + k];
        }
        __syncthreads();
    }
    // ---- Y = L B^-1: per row i of L solve C z = l_i, C^T y = z, in place in column i of Lt (coalesced over i;
    // the factor is read uniformly: LDS broadcast)
    for (int i = tid; i < n; i += nt) {
        for (int k = 0; k < r; ++k) {
            const int kk = k * (k + 1) / 2;
            double s0 = Lt[(int64_t)k * n + i], s1 = 0.0;
            int j = 0;
            for (; j + 1 < k; j += 2) {
                s0 -= Cp[kk + j] * Lt[(int64_t)j * n + i];
                s1 -= Cp[kk + j + 1] * Lt[(int64_t)(j + 1) * n + i];
            }
            if (j < k) s0 -= Cp[kk + j] * Lt[(int64_t)j * n + i];
            Lt[(int64_t)k * n + i] = (s0 + s1) / Cp[kk + k];
        }
        for (int k = r - 1; k >= 0; --k) {
            double s0 = Lt[(int64_t)k * n + i], s1 = 0.0;
            int j = k + 1;
            for (; j + 1 < r; j += 2) {
                s0 -= Cp[j * (j + 1) / 2 + k] * Lt[(int64_t)j * n + i];
                s1 -= Cp[(j + 1) * (j + 2) / 2 + k] * Lt[(int64_t)(j + 1) * n + i];
            }
            if (j < r) s0 -= Cp[j * (j + 1) / 2 + k] * Lt[(int64_t)j * n + i];
            Lt[(int64_t)k * n + i] = (s0 + s1) / Cp[k * (k + 1) / 2 + k];
        }
    }
    __syncthreads();
    // ---- eigen format: Vs = V = Y row-major, zero padded   (W is free now; Lt is read before it is overwritten)
    for (int idx = tid; idx < n * n; idx += nt) {
        const int i = idx / n, k = idx % n;
        W[idx] = k < r ? Lt[(int64_t)k * n + i] : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += nt) Lt[idx] = W[idx];
    if (tid == 0) e.chol_ok[b] = 2;
}
static __global__ __launch_bounds__(EIGH_THREADS) void pchol_pinv_kernel(EighArgs e, double lo, double hi, int lds_rank) {
    pchol_pinv_body(e, blockIdx.x, lo, hi, lds_rank);
}

// ------------------------------------------------------------------------------------------
// The same deflation over SEVERAL workgroups, for orders above 256 (round 6; pchol_pinv_kernel takes 19.5 ms at order 512 /
// rank 256 and 146 ms at 1023 / 512 in its one workgroup -- the case reference tests/test_n_run.py:14 constructs: rank >
// objects).  One launch per BLOCK of up to 32 pivots, grid = (matrices, slabs of 64 rows), no grid barrier: a launch reads
// one copy of the remaining diagonal / the state and writes the other, every workgroup repeats the small serial part
// (the 32 largest remaining diagonal entries by rank counting, their 32 x 32 block of the Schur complement, its Cholesky
// factorisation with REJECTION of pivots that fell to the noise level inside the block) and owns the rows of its slab:
//     C[i][p] = A[i][piv_p] - sum_{k < r} L[i][k] L[piv_p][k]      (the lazily evaluated columns, as pchol_pinv_kernel)
//     L[i][r + a] = (C[i][p_a] - sum_{b < a} L[i][r + b] Lb[a][b]) / Lb[a][a]      for the accepted pivots p_0 < p_1 < ...
//     d[i] -= sum_a L[i][r + a]^2
// Same acceptance rule and the same gap test as the one-workgroup kernel (pivot > lo * d_max; an accepted pivot below
// hi * d_max leaves the matrix to the eigen-solver); the CANDIDATES of a block are the 32 largest entries of the diagonal as
// it stood before the block, inside the block the pivots follow the current Schur complement (complete pivoting over the
// candidates): the factor differs from the one-workgroup kernel's, A = L L^T and the pseudo-inverse do not.  The host issues 2 ceil(n / 32) + 1 launches blind -- a launch whose matrix is finished, or was
// inverted by the fast path, returns at once --, then
//     pchol_verdict_kernel   gate[b] = the deflation finished cleanly; n_defl[b] = its order (0: the finishing launches idle)
//     B = L^T L (+ 1 on the diagonal beyond the rank)      gated product, pchol_patch_kernel
//     B^-1                                                  the blocked sweep of the fast path (sweep_step_kernel<BIG>) on B
//     Y^T = B^-1 L^T ,  K = Y Y^T                           gated products, straight into the K slot
//     pchol_done_kernel      chol_ok[b] = 1
// Order 512 / rank 256: see profiles/ (tools/bench_pinv.py).  A matrix the route declines at any point keeps chol_ok = 0 and
// falls to pchol_pinv_kernel / the eigen-solver exactly as before.
// ------------------------------------------------------------------------------------------
constexpr int DEFL_NB = 32, DEFL_ROWS = 64, DEFL_KC = 32, DEFL_THREADS = 256;
struct DeflArgs {
    double* d;         // [batch][2][EIGH_MAXN]  remaining diagonal (< 0: the index has been a pivot), two copies
    double* vals;      // [batch][2][2]          d_max of the input, smallest accepted pivot
    int* state;        // [batch][2][2]          rank so far, done (0 running, 1 finished, 2 declined: ambiguous spectrum)
    int* n_defl;       // [batch]                order for the finishing launches (0 = none)
    int* gate;         // [batch]                1 = finishing products run
    int* ok2;          // [batch]                verdict of the sweep over B
    int* rank;         // [batch]                numerical rank (information; tests)
};

static __global__ __launch_bounds__(256) void pchol_init_kernel(EighArgs e, DeflArgs da) {     // L = 0 for the matrices the fast path declined
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) { da.gate[b] = 0; da.n_defl[b] = 0; da.ok2[b] = 0; da.rank[b] = -1; }
    if (e.chol_ok[b] != 0) return;
    const int ld = e.n[b];
    double* Lt = e.V + (int64_t)b * e.stride;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < ld * ld; idx += gridDim.x * blockDim.x) Lt[idx] = 0.0;
}

static __global__ __launch_bounds__(DEFL_THREADS) void pchol_step_kernel(EighArgs e, DeflArgs da, double lo, double hi, int step) {
    __shared__ double sd[EIGH_MAXN];
    __shared__ double Lp[DEFL_KC][DEFL_NB + 1];        // L[piv_p][k0 + kk]
    __shared__ double Ls[DEFL_KC][DEFL_ROWS + 1];      // L[row0 + i][k0 + kk]
    __shared__ double Cp[DEFL_NB][DEFL_NB + 1];        // pivot block, then its Cholesky factor (accepted pivots)
    __shared__ double Cs[DEFL_ROWS][DEFL_NB + 1];      // panel of the slab, then its rows of L
    __shared__ double red[DEFL_THREADS / 64];
    __shared__ int piv[DEFL_NB], ord[DEFL_NB], open_[DEFL_NB], seq[DEFL_NB], s_elig, s_pick;
    const int b = blockIdx.x;
    if (e.chol_ok[b] != 0) return;                                          // (uniform: the fast path inverted this matrix)
    const int n = e.n_orig[b], ld = e.n[b];
    const int row0 = blockIdx.y * DEFL_ROWS;
    if (row0 >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int in = step & 1, out = in ^ 1;
    const double* A = e.A + (int64_t)b * e.stride;
    double* Lt = e.V + (int64_t)b * e.stride;                               // Lt[k * ld + i] = L[i][k]
    const double* din = da.d + ((int64_t)b * 2 + in) * EIGH_MAXN;
    double* dout = da.d + ((int64_t)b * 2 + out) * EIGH_MAXN;
    const int* sin = da.state + (b * 2 + in) * 2;
    int* sout = da.state + (b * 2 + out) * 2;
    const double* vin = da.vals + (b * 2 + in) * 2;
    double* vout = da.vals + (b * 2 + out) * 2;
    int r = 0, done = 0;
    double dmax0 = 0.0, last = __builtin_inf();
    if (step == 0) {
        double mx = 0.0;
        for (int i = tid; i < n; i += DEFL_THREADS) {
            const double v = A[(int64_t)i * ld + i];
            sd[i] = v;
            mx = fmax(mx, v);
        }
        for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
        if (lane == 0) red[wave] = mx;
        __syncthreads();
        dmax0 = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    } else {
        r = sin[0];
        done = sin[1];
        dmax0 = vin[0];
        last = vin[1];
        if (!done)
            for (int i = tid; i < n; i += DEFL_THREADS) sd[i] = din[i];
    }
    if (done) {                                                             // (uniform) finished in an earlier launch: hand the state on
        if (blockIdx.y == 0 && tid == 0) { sout[0] = r; sout[1] = done; vout[0] = dmax0; vout[1] = last; }
        return;
    }
    if (tid == 0) s_elig = 0;
    if (tid < DEFL_NB) { piv[tid] = 0; ord[tid] = -1; }
    __syncthreads();
    // ---- the (up to) 32 largest eligible entries of the remaining diagonal, by rank counting (ties: the smaller index first)
    const double thr = lo * dmax0;
    for (int i = tid; i < n; i += DEFL_THREADS) {
        const double v = sd[i];
        if (v > thr && v > 0.0) {
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const double w = sd[j];
                rank += (w > v || (w == v && j < i)) ? 1 : 0;
            }
            if (rank < DEFL_NB) piv[rank] = i;
            atomicAdd(&s_elig, 1);
        }
    }
    __syncthreads();
    const int m = s_elig < DEFL_NB ? s_elig : DEFL_NB;
    if (m == 0) {                                                           // (uniform) nothing left above the noise level: finished
        if (blockIdx.y == 0 && tid == 0) {
            sout[0] = r;
            sout[1] = (r > 0 && last < hi * dmax0) ? 2 : 1;
            vout[0] = dmax0;
            vout[1] = last;
        }
        return;
    }
    // ---- panel of the slab and pivot block, lazily: C = A[:, piv] - L[:, :r] L[piv, :r]^T
    const int tx = tid & 31, ty = tid >> 5;                                // column p = tx; rows ty, ty + 8, ...
    double cs[DEFL_ROWS / 8], cp[DEFL_NB / 8];
    const int pc = tx < m ? piv[tx] : piv[0];
#pragma unroll
    for (int q = 0; q < DEFL_ROWS / 8; ++q) {
        const int i = row0 + ty + 8 * q;
        cs[q] = (i < n && tx < m) ? A[(int64_t)i * ld + pc] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < DEFL_NB / 8; ++q) {
        const int pr = ty + 8 * q;
        cp[q] = (pr < m && tx < m) ? A[(int64_t)piv[pr] * ld + pc] : 0.0;
    }
    for (int k0 = 0; k0 < r; k0 += DEFL_KC) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < DEFL_KC / 8; ++q) {                             // Lp[kk][p]: kk = ty + 8 q, p = tx
            const int kk = ty + 8 * q;
            Lp[kk][tx] = (k0 + kk < r && tx < m) ? Lt[(int64_t)(k0 + kk) * ld + pc] : 0.0;
        }
        {
            const int i = tid & 63;
#pragma unroll
            for (int q = 0; q < DEFL_KC / 4; ++q) {                         // Ls[kk][i]: kk = (tid >> 6) + 4 q
                const int kk = (tid >> 6) + 4 * q;
                Ls[kk][i] = (k0 + kk < r && row0 + i < n) ? Lt[(int64_t)(k0 + kk) * ld + row0 + i] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < DEFL_KC; ++kk) {
            const double lp = Lp[kk][tx];
#pragma unroll
            for (int q = 0; q < DEFL_ROWS / 8; ++q) cs[q] -= Ls[kk][ty + 8 * q] * lp;
#pragma unroll
            for (int q = 0; q < DEFL_NB / 8; ++q) cp[q] -= Lp[kk][ty + 8 * q] * lp;
        }
    }
#pragma unroll
    for (int q = 0; q < DEFL_ROWS / 8; ++q) Cs[ty + 8 * q][tx] = cs[q];
#pragma unroll
    for (int q = 0; q < DEFL_NB / 8; ++q) Cp[ty + 8 * q][tx] = cp[q];
    __syncthreads();
    // ---- Cholesky of the pivot block with COMPLETE pivoting inside the block: the next pivot is the largest current diagonal
    // entry among the block's open candidates (the candidates were picked by the diagonal as it stood before the block; inside
    // it the order follows the Schur complement, as in the one-workgroup kernel), and what the block's earlier pivots took
    // below the noise level is rejected (it stays an ordinary row; its updated diagonal keeps it from being chosen again).
    // Cp keeps full symmetric storage of the open part; column a-th-pivot of Cp holds that column of the factor.
    int n_acc = 0;
    if (tid < DEFL_NB) { open_[tid] = tid < m ? 1 : 0; seq[tid] = 0; }
    __syncthreads();
    for (int t = 0; t < m; ++t) {
        if (tid == 0) {
            int best = -1;
            double bv = thr;
            for (int q = 0; q < m; ++q)
                if (open_[q] && Cp[q][q] > bv && Cp[q][q] > 0.0) { bv = Cp[q][q]; best = q; }
            s_pick = best;
        }
        __syncthreads();
        const int q0 = s_pick;
        if (q0 < 0) break;                                                  // (uniform) the rest of the block is noise
        const double pv = Cp[q0][q0], lkk = sqrt(pv);
        __syncthreads();
        if (tid < m && tid != q0 && open_[tid]) Cp[tid][q0] /= lkk;
        __syncthreads();
        for (int idx = tid; idx < m * m; idx += DEFL_THREADS) {
            const int q = idx / m, c = idx % m;
            if (q != q0 && c != q0 && open_[q] && open_[c]) Cp[q][c] -= Cp[q][q0] * Cp[c][q0];
        }
        __syncthreads();
        if (tid == 0) { Cp[q0][q0] = lkk; open_[q0] = 0; ord[q0] = n_acc; seq[n_acc] = q0; }
        ++n_acc;
        last = fmin(last, pv);
        __syncthreads();
    }
    __syncthreads();
    // ---- the slab's rows of the new columns of L (column r + a belongs to the a-th accepted pivot, candidate seq[a]), the
    // remaining diagonal
    if (tid < DEFL_ROWS && row0 + tid < n) {
        const int i = row0 + tid;
        const double di = sd[i];
        int own = -1;                                                       // this row is an accepted pivot of the block: its candidate index
        for (int p = 0; p < m; ++p)
            if (piv[p] == i && ord[p] >= 0) own = p;
        double sq = 0.0;
        for (int a = 0; a < n_acc; ++a) {
            const int ca = seq[a];
            double x;
            if (di < 0.0) x = 0.0;                                          // a pivot of an earlier block: above the diagonal
            else if (own >= 0) x = a < ord[own] ? Cp[own][ca] : (a == ord[own] ? Cp[own][own] : 0.0);   // its row of the factor
            else {
                double sacc = Cs[tid][ca];
                for (int bb = 0; bb < a; ++bb) sacc -= Cs[tid][seq[bb]] * Cp[ca][seq[bb]];
                x = sacc / Cp[ca][ca];
            }
            Cs[tid][ca] = x;
            sq += x * x;
            Lt[(int64_t)(r + a) * ld + i] = x;
        }
        double nd = di;
        if (own >= 0) nd = -1.0;
        else if (di >= 0.0) { nd = di - sq; nd = nd > 0.0 ? nd : 0.0; }
        dout[i] = nd;
    }
    if (blockIdx.y == 0 && tid == 0) {
        sout[0] = r + n_acc;
        sout[1] = 0;
        vout[0] = dmax0;
        vout[1] = last;
    }
}

// after the last step: did the deflation finish cleanly?  (final = the copy of the state the last launch wrote)
static __global__ __launch_bounds__(64) void pchol_verdict_kernel(EighArgs e, DeflArgs da, int final_copy) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int* s = da.state + (b * 2 + final_copy) * 2;
    const bool ok = e.chol_ok[b] == 0 && s[1] == 1;
    da.gate[b] = ok ? 1 : 0;
    da.n_defl[b] = ok ? e.n_orig[b] : 0;
    da.rank[b] = e.chol_ok[b] == 0 ? s[0] : -1;
}
// B = L^T L has rank r: 1 on the diagonal beyond it makes the matrix the sweep inverts positive definite (the block beyond r
// is the identity and stays decoupled: L's columns there are zero)
static __global__ __launch_bounds__(256) void pchol_patch_kernel(EighArgs e, DeflArgs da, int final_copy) {
    const int b = blockIdx.x;
    if (!da.gate[b]) return;
    const int n = e.n_orig[b], ld = e.n[b], r = da.state[(b * 2 + final_copy) * 2];
    double* B = e.Vs + (int64_t)b * e.stride;
    for (int k = r + threadIdx.x; k < n; k += blockDim.x) B[(int64_t)k * ld + k] = 1.0;
}
static __global__ __launch_bounds__(64) void pchol_done_kernel(EighArgs e, DeflArgs da) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0 && da.gate[b] && da.ok2[b] == 1) e.chol_ok[b] = 1;
}
// the gate of the products behind the sweep over B: both verdicts
static __global__ __launch_bounds__(64) void pchol_gate2_kernel(DeflArgs da) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0) da.gate[b] = (da.gate[b] && da.ok2[b] == 1) ? 1 : 0;
}

// Pack / unpack between the caller's matrices and the eigen workspace, batched (blockIdx.y = matrix): the per-type launches
// of one pseudo-inverse pass collapse into one launch each -- on small graphs an iteration is bounded by the number of
// dependent launches, not by their work.  T = element type of the caller's matrices (the plan: f64, ld = c; the stand-alone
// operator: f64 / f32 with the caller's leading dimensions).  The sweep kernels write K themselves: f64 only.
constexpr int PINV_MAXB = 16;
struct PinvBatch {
    const void* gram[PINV_MAXB];     // c x c, leading dimension ldg
    void* K[PINV_MAXB];              // c x c, leading dimension ldk
    int64_t ldg[PINV_MAXB], ldk[PINV_MAXB];
    int c[PINV_MAXB], n_pad[PINV_MAXB];
};

// pad helper for the eigen workspace: A + b * stride (f64, n_pad x n_pad) <- gram[b] (T, n x n);
// the padding row/column is decoupled (zero off-diagonal, zero diagonal -> eigenvalue 0).
template <typename T>
__global__ __launch_bounds__(256) void eigh_pack_kernel(PinvBatch pb, double* __restrict__ A, int64_t stride,
                                                        int* __restrict__ n_pad_out = nullptr,
                                                        int* __restrict__ n_out = nullptr) {
    const int b = blockIdx.y, n = pb.c[b], n_pad = pb.n_pad[b];
    // (the stand-alone operator has no bind step that could upload the two orders: written here, the call needs neither
    //  host-to-device copies nor a stream synchronisation)
    if (n_pad_out && blockIdx.x == 0 && threadIdx.x == 0) {
        n_pad_out[b] = n_pad;
        n_out[b] = n;
    }
    double* dst = A + (int64_t)b * stride;
    const T* src = (const T*)pb.gram[b];
    const int64_t lds = pb.ldg[b];
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n_pad * n_pad; idx += gridDim.x * blockDim.x) {
        const int r = idx / n_pad, c = idx % n_pad;
        dst[idx] = (r < n && c < n) ? (double)src[(int64_t)r * lds + c] : 0.0;
    }
}

// K(r,c) = sum_{k >= max(r,c)} X(k,r) X(k,c)   (inverse from the inverted Cholesky factor)
template <typename T>
__global__ __launch_bounds__(256) void chol_unpack_kernel(PinvBatch pb, const double* __restrict__ Xall, int64_t stride,
                                                          const int* __restrict__ chol_ok) {
    const int b = blockIdx.y;
    if (chol_ok[b] != 1) return;
    const int n = pb.c[b], ld = pb.n_pad[b];
    const double* X = Xall + (int64_t)b * stride;
    T* K = (T*)pb.K[b];
    const int64_t ldk = pb.ldk[b];
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n * n; idx += gridDim.x * blockDim.x) {
        const int r = idx / n, c = idx % n;
        double s = 0.0;
        for (int k = (r > c ? r : c); k < n; ++k) s += X[k * ld + r] * X[k * ld + c];
        K[(int64_t)r * ldk + c] = (T)s;
    }
}

// ------------------------------------------------------------------------------------------
// Fast path of the pseudo-inverse for orders 65 .. SWEEP_MAXN (round 4): K = A^-1 of a symmetric positive definite matrix by
// the BLOCKED SWEEP OPERATOR, one workgroup of 512 threads per matrix, straight into the K slot -- no factor, no triangular
// inverse, no X^T X product behind it (chol_inverse_blocked_kernel + chol_unpack: 1.15 + 0.09 ms at order 256, and the
// critical path of a rank of the ownership-sharded iteration and of config 5's pipeline; this kernel: see profiles/).
// Sweeping pivot k of a symmetric M: m_ij -= c_i c_j / m_kk (c = column k), row / column k <- c / m_kk, m_kk <- -1 / m_kk;
// after all n pivots M = -A^-1.  Blocked by NB = 32 pivots: with P = M_pp^-1 of the CURRENT pivot block
//     M_rr -= M_rp P M_pr ,  M_rp <- M_rp P ,  M_pr <- P M_pr ,  M_pp <- -P
// (sweeping a block is sweeping its pivots one after the other).  Per block: the panel C = M[:, block] and the pivot block
// go to LDS; the 32 x 32 block is swept pivot by pivot with ONE barrier per pivot (two elements per thread in registers,
// row k published through a double buffer) -- its pivots are the Schur complements a Cholesky factorisation would take the
// roots of, so the verdict is that of the Cholesky kernels: pivot > rel_thr * a_kk, a_kk above the diagonal floor; a failed
// pivot leaves the matrix (untouched in e.A) to the deflation / eigen-solver --; T = M_rp P (n x 32) and the rank-32 update
// of the whole matrix run on the f64 matrix cores (16 x 16 x 4 tiles, operands from LDS at a pitch of 36 words: conflict-free
// fragments; a wave owns 64 x 64 outputs of the update at a time, its accumulators start from M itself).  On this part the
// vector ALU and the matrix cores run f64 FMAs at the same rate (78.6 TFLOP/s either way: 13.7 us per block on one CU at
// order 256); what the matrix cores save is LDS traffic -- the plain-FMA T read two LDS words per FMA and took 14 of the
// 66 us of a block (time stamps of a probe build, -DSKF_PROBE_STAMPS).  M lives in the plan's eigen scratch (e.V), 0.5 MB:
// L2 resident.  Stand-alone at order 256: 0.53 ms (first version 0.63; Cholesky inverse + unpack 0.93) -- per block: panel
// 2 us, pivot-block sweep 14, T 2.6, update 27, write-back 7.
// ------------------------------------------------------------------------------------------
constexpr int SWEEP_MAXN = 256;
constexpr int SWEEP_NB = 32;
constexpr int SWEEP_LD = SWEEP_NB + 4;      // (row r, k) -> 4 r + k mod 32: the fragments of the matrix-core tiles are conflict-free
constexpr int SWEEP_THREADS = 512;
constexpr int SWEEP_LDS_BYTES = ((2 * SWEEP_MAXN + SWEEP_NB) * SWEEP_LD + 6 * SWEEP_NB + SWEEP_MAXN) * 8;

// The sweep of one 32 x 32 pivot block by ONE wave (round 5, sweep_step_kernel): lane = (column c = lane & 31, half =
// lane >> 5) holds rows 16 half .. 16 half + 15 of its column in registers; row k of the current state travels through LDS
// (double-buffered) and the wave orders its own LDS traffic -- no workgroup barrier per pivot.  (sweep_inverse_kernel spreads
// the block over its 512 threads, two elements each, with one __syncthreads() per pivot: 14 us per block -- barriers and LDS
// round trips, not the 2 k FMAs.)  The chain from one pivot to the next is: element of row k + 1 -> LDS -> every lane ->
// reciprocal -> update; so pivot k updates ROW k + 1 FIRST, the lane that holds the next pivot takes its reciprocal at once,
// row and reciprocal go to LDS, and the other 15 rows of the lane are updated while that round trip is in flight.  The loop
// has no data-dependent branch: a failed pivot clears `ok` and the arithmetic runs on (its results are dropped).  The
// padding of a short block (rows / columns >= nb) is zero on entry and stays +0 under every finite pivot, so nothing masks
// it inside the loop.  The arithmetic of an element is the same expression in the same order as in sweep_inverse_kernel
// (1 / pivot is the same IEEE quotient whichever lane takes it), so the bits are the same.
// rowk: SWEEP_ROWK_WORDS words.  Returns false when a pivot failed its bound (uniform).
constexpr int SWEEP_ROWK = 2 * SWEEP_NB;          // a row of the pivot block and, behind it, the reciprocals of its elements
constexpr int SWEEP_ROWK_WORDS = 3 * SWEEP_ROWK;  // two buffers and one nobody reads
__device__ __forceinline__ bool sweep_pivot_block(const double* __restrict__ Cblk, double* __restrict__ Pv,
                                                  double* __restrict__ rowk, const double* __restrict__ need, int nb, int lane) {
    constexpr int NB = SWEEP_NB, LD = SWEEP_LD, RK = SWEEP_ROWK;
    const int c = lane & 31, half = lane >> 5;
    double v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int r = 16 * half + q;
        v[q] = (r < nb && c < nb) ? Cblk[r * LD + c] : 0.0;
    }
    // every lane stores what it has of row k + 1 and the reciprocal of it -- the half that does not hold the row into a
    // buffer nobody reads: no branch, and the quotient is scheduled among the updates of the other rows
    {
        double* dst = rowk + (half == 0 ? 0 : 2 * RK);
        dst[c] = v[0];
        dst[NB + c] = 1.0 / v[0];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    bool ok = true;
#pragma unroll
    for (int k = 0; k < NB; ++k) {                                       // (a fixed trip count: the registers of v are named)
        if (k < nb) {                                                    // (uniform)
            const double* rk = rowk + (k & 1) * RK;
            const double piv = rk[k];                                    // (every lane reads the same words)
            ok = ok & (piv > need[k]);
            const double d = rk[NB + k];
            const double cc = rk[c];
            double e[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) e[q] = rk[16 * half + q] * d;
            auto swept = [&](int q) -> double {
                const double gen = (c == k) ? e[q] : fma(-e[q], cc, v[q]);
                if (q != (k & 15)) return gen;
                const double piv_row = (c == k) ? -d : cc * d;           // row k itself, in the half that holds it
                return (half == (k >> 4)) ? piv_row : gen;
            };
            const int q1 = (k + 1) & 15;                                 // row k + 1 first: it carries the next pivot
            if (k + 1 < NB) {
                v[q1] = swept(q1);
                double* dst = rowk + (half == ((k + 1) >> 4) ? ((k + 1) & 1) * RK : 2 * RK);
                dst[c] = v[q1];
                dst[NB + c] = 1.0 / v[q1];
            }
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (!(k + 1 < NB && q == q1)) v[q] = swept(q);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) Pv[(16 * half + q) * LD + c] = v[q];
    return ok;
}

static __global__ __launch_bounds__(SWEEP_THREADS) void sweep_inverse_kernel(EighArgs e, PinvBatch pb, double rel_thr) {
    constexpr int NB = SWEEP_NB, LD = SWEEP_LD;
    HIP_DYNAMIC_SHARED(double, ssm)
    __shared__ double red[SWEEP_THREADS / 64];
    __shared__ double s_max;
    double* Cs = ssm;                              // [SWEEP_MAXN][LD]  panel C = M[:, kb .. kb + nb)
    double* Ts = Cs + SWEEP_MAXN * LD;             // [SWEEP_MAXN][LD]  T = M_rp P
    double* Pv = Ts + SWEEP_MAXN * LD;             // [NB][LD]          the swept pivot block: -P
    double* rowk = Pv + NB * LD;                   // [2][NB]           row k of the pivot block, double-buffered (6 NB words reserved)
    double* need = rowk + 6 * NB;                  // [SWEEP_MAXN]      the bound pivot k has to exceed
    const int b = blockIdx.x;
    const int n = e.n_orig[b], ld = e.n[b];
    if (n > SWEEP_MAXN) return;                    // (the host sends such plans to chol_inverse_blocked_kernel)
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;      // 32 x 16
    const int lane = tid & 63, wave = tid >> 6;
    const double* A = e.A + (int64_t)b * e.stride;
    double* M = e.V + (int64_t)b * e.stride;

    double mx = 0.0;
    for (int idx = tid; idx < n * n; idx += SWEEP_THREADS) {
        const int r = idx / n, c = idx % n;
        const double v = 0.5 * (A[r * ld + c] + A[c * ld + r]);
        M[r * ld + c] = v;
        if (r == c) mx = fmax(mx, fabs(v));
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < SWEEP_THREADS / 64; ++i) s = fmax(s, red[i]);
        s_max = s;
    }
    __syncthreads();
    {   // the three tests on pivot k -- a_kk > floor, pivot > thr a_kk, pivot > 0 -- as ONE bound (+inf where a_kk fails)
        const double floor_ = chol_diag_floor(n) * s_max;
        for (int k = tid; k < n; k += SWEEP_THREADS) {
            const double akk = A[k * ld + k];
            need[k] = (akk > floor_) ? fmax(rel_thr * akk, 0.0) : __builtin_inf();
        }
    }
    __syncthreads();

#ifdef SKF_PROBE_STAMPS
    long long ph[6] = {0, 0, 0, 0, 0, 0}, t_in = wall_clock64();
#define SKF_STAMP(i) { const long long now_ = wall_clock64(); ph[i] += now_ - t_in; t_in = now_; }
#else
#define SKF_STAMP(i)
#endif
    for (int kb = 0; kb < n; kb += NB) {
        const int nb = (n - kb < NB) ? n - kb : NB;
        SKF_STAMP(0)
        // ---- panel and pivot block to LDS
        for (int i = ty; i < n; i += 16) Cs[i * LD + tx] = (tx < nb) ? M[i * ld + kb + tx] : 0.0;
        __syncthreads();
        SKF_STAMP(1)
        // ---- sweep of the pivot block: elements (r, c) = (ty, tx) and (ty + 16, tx) in registers
        double v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = ty + 16 * h;
            v[h] = (r < nb && tx < nb) ? Cs[(kb + r) * LD + tx] : 0.0;
        }
        if (ty == 0) rowk[tx] = v[0];                                    // row 0
        __syncthreads();
        bool ok = true;
        for (int k = 0; k < nb; ++k) {
            const double* rk = rowk + (k & 1) * NB;
            const double piv = rk[k];
            if (!(piv > need[kb + k])) {                                 // (uniform: every thread reads the same words)
                ok = false;
                break;
            }
            const double d = 1.0 / piv;
            const double cc = rk[tx];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = ty + 16 * h;
                const double cr = rk[r];
                const double nv = (r == k) ? ((tx == k) ? -d : cc * d) : ((tx == k) ? cr * d : fma(-cr * d, cc, v[h]));
                v[h] = (r < nb && tx < nb) ? nv : 0.0;
                if (r == k + 1) rowk[((k + 1) & 1) * NB + tx] = v[h];     // row k + 1 of the swept block, for the next pivot
            }
            __syncthreads();
        }
        if (!ok) {                                                       // (uniform)
            if (tid == 0) e.chol_ok[b] = 0;
            return;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) Pv[(ty + 16 * h) * LD + tx] = v[h];
        __syncthreads();
        SKF_STAMP(2)
        // ---- T = M_rp P = -(C Pv), every row (the pivot rows' entries are not used), on the f64 matrix cores: 16 x 16 tiles,
        // row tiles wave, wave + 8, both column tiles on one A fragment.  (The plain-FMA form read two LDS words per FMA: 4 MB
        // per block, 14 of the 66 us a block took at order 256 -- time stamps of a probe build.)
        {
            typedef Mfma<double> MF;
            const int ntile = (n + 15) >> 4;
            for (int it = wave; it < ntile; it += SWEEP_THREADS / 64) {
                const int row = it * 16 + MF::a_row(lane);
                MF::acc_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k0 = 0; k0 < NB; k0 += MF::KT) {
                    const int kk = k0 + MF::ab_k(lane);
                    const double a = row < n ? Cs[row * LD + kk] : 0.0;
                    acc0 = MF::mma(a, Pv[kk * LD + MF::a_row(lane)], acc0);
                    acc1 = MF::mma(a, Pv[kk * LD + 16 + MF::a_row(lane)], acc1);
                }
#pragma unroll
                for (int r = 0; r < MF::NREG; ++r) {
                    const int i = it * 16 + MF::d_row(lane, r);
                    if (i < n) {
                        Ts[i * LD + MF::d_col(lane)] = -acc0[r];
                        Ts[i * LD + 16 + MF::d_col(lane)] = -acc1[r];
                    }
                }
            }
        }
        __syncthreads();
        SKF_STAMP(3)
        // ---- M_rr -= T C^T outside the pivot rows / columns, on the f64 matrix cores: a wave owns 64 x 64 outputs at a time
        // (4 x 4 tiles on four A and four B fragments per K step: 8 LDS reads for 16 instructions; 8 x 8 outputs per thread
        // in plain FMAs read 16 words per 64 FMAs and ran on the LDS, 27 us per block at order 256)
        {
            typedef Mfma<double> MF;
            const int nblk = (n + 63) >> 6;
            for (int blk = wave; blk < nblk * nblk; blk += SWEEP_THREADS / 64) {
                const int bi = (blk / nblk) * 64, bj = (blk % nblk) * 64;
                // the accumulators start from M itself (the loads fly while the first products run) and take -T C^T
                MF::acc_t acc[4][4];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < MF::NREG; ++r) {
                        const int i = bi + 16 * a + MF::d_row(lane, r);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int j = bj + 16 * q + MF::d_col(lane);
                            acc[a][q][r] = (i < n && j < n) ? M[i * ld + j] : 0.0;
                        }
                    }
#pragma unroll 2
                for (int k0 = 0; k0 < NB; k0 += MF::KT) {
                    const int kk = k0 + MF::ab_k(lane);
                    double ta[4], cb[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const int i = bi + 16 * a + MF::a_row(lane);
                        ta[a] = i < n ? -Ts[i * LD + kk] : 0.0;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int j = bj + 16 * q + MF::a_row(lane);
                        cb[q] = j < n ? Cs[j * LD + kk] : 0.0;
                    }
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[a][q] = MF::mma(ta[a], cb[q], acc[a][q]);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < MF::NREG; ++r) {
                        const int i = bi + 16 * a + MF::d_row(lane, r);
                        if (i >= n || (i >= kb && i < kb + nb)) continue;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int j = bj + 16 * q + MF::d_col(lane);
                            if (j < n && !(j >= kb && j < kb + nb)) M[i * ld + j] = acc[a][q][r];
                        }
                    }
            }
        }
        SKF_STAMP(4)
        // ---- pivot columns <- T (lanes along the columns of the block), pivot block <- -P; pivot rows <- T^T with the lanes
        // along the rows of T (the transposed copy as the mirror of the column loop: one 8-byte store per lane ld apart,
        // 9 of the 66 us)
        for (int i = ty; i < n; i += 16) {
            if (tx >= nb) continue;
            if (i >= kb && i < kb + nb) M[i * ld + kb + tx] = Pv[(i - kb) * LD + tx];
            else M[i * ld + kb + tx] = Ts[i * LD + tx];
        }
        for (int idx = tid; idx < nb * n; idx += SWEEP_THREADS) {
            const int c = idx / n, i = idx % n;
            if (!(i >= kb && i < kb + nb)) M[(kb + c) * ld + i] = Ts[i * LD + c];
        }
        __syncthreads();
    }
    SKF_STAMP(5)
#ifdef SKF_PROBE_STAMPS
    if (tid == 0 && n >= 200)
        printf("sweep_inverse n %d: panel load %lld, pivot block sweep %lld, T %lld, update %lld, write-back + barrier %lld (x10 ns, all blocks)\n", n,
               ph[1], ph[2], ph[3], ph[4], ph[5] + ph[0]);
#endif
    // ---- all pivots swept: M = -A^-1
    double* K = (double*)pb.K[b];
    for (int idx = tid; idx < n * n; idx += SWEEP_THREADS) K[idx] = -M[(idx / n) * ld + idx % n];
    if (tid == 0) e.chol_ok[b] = 1;
}

// ------------------------------------------------------------------------------------------
// The same sweep with the rank-32 update of a block step spread over SEVERAL workgroups (round 5): one launch per block
// step, grid = (matrices, row slabs).  A slab is `rs` rows of the matrix (a multiple of 32); its workgroup repeats the small
// serial part of the step -- panel to LDS, the pivot-block sweep by one wave -- and then owns everything that carries one of
// its rows i: T_i = M_ip P, the updated M_ij, the pivot columns (i, p) and, transposed, the pivot rows (p, i); the slab that
// holds the pivot rows also writes -P.  A step READS one copy of the matrix and WRITES the other (e.V / e.Vs alternate; the
// first step reads the symmetrised input itself, the last one writes K = -M), so no workgroup waits for another inside a
// launch and there is no grid barrier to hang on: the order between steps is the stream's.  Every element takes the
// arithmetic of sweep_inverse_kernel in the same order (the accumulators of a tile start from M and run over the 32 pivots
// in steps of four) -- the two kernels return the same bits.  chol_ok[b] carries the state between launches: 3 = steps so
// far accepted every pivot, 0 = a pivot failed (the later steps of that matrix return at once; e.A is untouched for the
// deflation / eigen-solver), 1 after the last step.
// One workgroup per matrix spends 53 us per block at order 256, 27 of them in the update; here a step is the serial part
// plus one 32 x 32 tile per wave, and a launch boundary (profiles/: tools/bench_pinv.py).
// ------------------------------------------------------------------------------------------
constexpr int SWEEP_RUNNING = 3;
// BIG (orders above SWEEP_MAXN, up to EIGH_MAXN): the panel of every row does not fit the LDS -- it holds the pivot rows and
// the rows of the slab only (slabs of exactly 32 rows); the column operands C_j of a tile come from the matrix in memory (L2:
// 8 MB at order 1024), asked for together with the tile's accumulators.  Same arithmetic, element by element.
constexpr int SWEEP_BIG_ROWS = 2 * SWEEP_NB;      // pivot rows, slab rows
constexpr int SWEEP_BIG_LDS_BYTES = ((SWEEP_BIG_ROWS + 2 * SWEEP_NB) * SWEEP_LD + 6 * SWEEP_NB + SWEEP_NB) * 8;

template <bool BIG>
__global__ __launch_bounds__(SWEEP_THREADS) void sweep_step_kernel(EighArgs e, PinvBatch pb, double rel_thr, int step, int rs) {
    constexpr int NB = SWEEP_NB, LD = SWEEP_LD;
    constexpr int CROWS = BIG ? SWEEP_BIG_ROWS : SWEEP_MAXN, TROWS = BIG ? SWEEP_NB : SWEEP_MAXN;
    constexpr int PCN = BIG ? SWEEP_BIG_ROWS / 16 : SWEEP_MAXN / 16;
    typedef Mfma<double> MF;
    HIP_DYNAMIC_SHARED(double, ssm)
    __shared__ double red[SWEEP_THREADS / 64];
    __shared__ int s_ok;
    double* Cs = ssm;                              // panel C = M[:, kb .. kb + nb): every row | BIG: pivot rows, then slab rows
    double* Ts = Cs + CROWS * LD;                  // T = M_rp P (rows of this slab)
    double* Pv = Ts + TROWS * LD;                  // [NB][LD]          the swept pivot block: -P
    double* rowk = Pv + NB * LD;                   // [SWEEP_ROWK_WORDS]
    double* need = rowk + 6 * NB;                  // [NB]              the bounds of this step's pivots
    const int b = blockIdx.x;
    const int n = e.n_orig[b], ld = e.n[b];
    const int kb = step * NB;
    if (n > (BIG ? EIGH_MAXN : SWEEP_MAXN) || kb >= n) return;
    if (BIG) rs = NB;
    const int r0 = blockIdx.y * rs, r1 = (r0 + rs < n) ? r0 + rs : n;
    if (r0 >= n) return;
    const bool first = step == 0, last = kb + NB >= n;
    if (!first && *(volatile const int*)(e.chol_ok + b) == 0) return;     // (uniform; slab 0 of THIS launch may already have written its verdict)
    const int nb = (n - kb < NB) ? n - kb : NB;
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;      // 32 x 16
    const int lane = tid & 63, wave = tid >> 6;
    const double* A = e.A + (int64_t)b * e.stride;
    const double* Min = ((step & 1) ? e.Vs : e.V) + (int64_t)b * e.stride;
    double* Mout = ((step & 1) ? e.V : e.Vs) + (int64_t)b * e.stride;
    double* K = (double*)pb.K[b];
    auto in = [&](int i, int j) -> double { return first ? 0.5 * (A[i * ld + j] + A[j * ld + i]) : Min[i * ld + j]; };
    auto out = [&](int i, int j, double v) {
        if (last) K[(int64_t)i * n + j] = -v;
        else Mout[i * ld + j] = v;
    };
    // rows of the panel / of T in LDS
    auto crow = [&](int i) -> int { return BIG ? NB + (i - r0) : i; };   // a row of the slab
    auto trow = [&](int i) -> int { return BIG ? i - r0 : i; };
    const int piv0 = BIG ? 0 : kb;                                       // first pivot row

#ifdef SKF_PROBE_STAMPS
    long long ph[6] = {0, 0, 0, 0, 0, 0}, t_in = wall_clock64();
#define SKF_STAMP(i) { const long long now_ = wall_clock64(); ph[i] += now_ - t_in; t_in = now_; }
#else
#define SKF_STAMP(i)
#endif
    // ---- everything the step reads from memory is asked for up front: the panel (every row: the columns j of the update
    // come from it | BIG: pivot rows and slab rows), the diagonal of the input for the bounds of this step's pivots (as
    // sweep_inverse_kernel), and the wave's first tile of M -- its loads fly while wave 0 sweeps the pivot block
    auto panel_row = [&](int u) -> int {                                 // the matrix row behind LDS row ty + 16 u (-1: none)
        const int l = ty + 16 * u;
        if (!BIG) return l < n ? l : -1;
        const int i = l < NB ? kb + l : r0 + (l - NB);
        return (l < NB ? l < nb : i < r1) ? i : -1;
    };
    double pc[PCN];
#pragma unroll
    for (int u = 0; u < PCN; ++u) {
        const int i = panel_row(u);
        pc[u] = (i >= 0 && tx < nb) ? in(i, kb + tx) : 0.0;
    }
    double mx = 0.0;
    for (int k = tid; k < n; k += SWEEP_THREADS) mx = fmax(mx, fabs(A[k * ld + k]));
    const double akk = tid < nb ? A[(kb + tid) * ld + kb + tid] : 0.0;
    const int ncol = (n + 31) >> 5, nrow = (r1 - r0 + 31) >> 5;
    auto tile_at = [&](int blk, int& bi, int& bj) -> bool {              // false: pivot rows / columns only (or past the end)
        bi = r0 + (blk / ncol) * 32;
        bj = (blk % ncol) * 32;
        return blk < nrow * ncol && bi != kb && bj != kb;
    };
    struct Tile {
        MF::acc_t acc[2][2];
        double cb[BIG ? NB / MF::KT : 1][2];                             // BIG: the column operands C_j of the tile, all K steps
    };
    auto tile_load = [&](int bi, int bj, Tile& t) {                      // the accumulators start from M itself
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < MF::NREG; ++r) {
                const int i = bi + 16 * a + MF::d_row(lane, r);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int j = bj + 16 * q + MF::d_col(lane);
                    t.acc[a][q][r] = (i < n && j < n) ? in(i, j) : 0.0;
                }
            }
        if (BIG) {
#pragma unroll
            for (int ks = 0; ks < NB / MF::KT; ++ks) {
                const int kk = ks * MF::KT + MF::ab_k(lane);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int j = bj + 16 * q + MF::a_row(lane);
                    t.cb[BIG ? ks : 0][q] = (j < n && kk < nb) ? in(j, kb + kk) : 0.0;
                }
            }
        }
    };
    Tile t0;
    int bi0, bj0;
    const bool have0 = tile_at(wave, bi0, bj0);
    if (have0) tile_load(bi0, bj0, t0);
#pragma unroll
    for (int u = 0; u < PCN; ++u) {
        const int l = ty + 16 * u;
        if (BIG || l < n) Cs[l * LD + tx] = pc[u];
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    SKF_STAMP(0)
    if (wave == 0) {
        double smax = 0.0;
#pragma unroll
        for (int i = 0; i < SWEEP_THREADS / 64; ++i) smax = fmax(smax, red[i]);
        if (tid < nb) need[tid] = (akk > chol_diag_floor(n) * smax) ? fmax(rel_thr * akk, 0.0) : __builtin_inf();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const bool ok = sweep_pivot_block(Cs + piv0 * LD, Pv, rowk, need, nb, lane);
        if (lane == 0) s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    SKF_STAMP(1)
    if (!s_ok) {                                                         // (uniform, and the same verdict in every slab)
        if (tid == 0 && blockIdx.y == 0) e.chol_ok[b] = 0;
        return;
    }
    // ---- T = -(C Pv) for the rows of the slab
    {
        const int t0r = r0 >> 4, t1r = (r1 + 15) >> 4;
        for (int it = t0r + wave; it < t1r; it += SWEEP_THREADS / 64) {
            const int row = it * 16 + MF::a_row(lane);
            MF::acc_t a0 = {0.0, 0.0, 0.0, 0.0}, a1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k0 = 0; k0 < NB; k0 += MF::KT) {
                const int kk = k0 + MF::ab_k(lane);
                const double a = row < r1 ? Cs[crow(row) * LD + kk] : 0.0;
                a0 = MF::mma(a, Pv[kk * LD + MF::a_row(lane)], a0);
                a1 = MF::mma(a, Pv[kk * LD + 16 + MF::a_row(lane)], a1);
            }
#pragma unroll
            for (int r = 0; r < MF::NREG; ++r) {
                const int i = it * 16 + MF::d_row(lane, r);
                if (i < r1) {
                    Ts[trow(i) * LD + MF::d_col(lane)] = -a0[r];
                    Ts[trow(i) * LD + 16 + MF::d_col(lane)] = -a1[r];
                }
            }
        }
    }
    __syncthreads();
    SKF_STAMP(2)
    // ---- M_ij - T_i C_j^T outside the pivot rows / columns: a wave owns 32 x 32 outputs at a time
    {
        auto tile_finish = [&](int bi, int bj, Tile& t) {
            auto kstep = [&](int k0) {
                const int kk = k0 + MF::ab_k(lane);
                double ta[2], cb[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int i = bi + 16 * a + MF::a_row(lane);
                    ta[a] = i < r1 ? -Ts[trow(i) * LD + kk] : 0.0;
                }
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int j = bj + 16 * q + MF::a_row(lane);
                    if (BIG) cb[q] = t.cb[BIG ? k0 / MF::KT : 0][q];
                    else cb[q] = j < n ? Cs[j * LD + kk] : 0.0;
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int q = 0; q < 2; ++q) t.acc[a][q] = MF::mma(ta[a], cb[q], t.acc[a][q]);
            };
            if (BIG) {                                                   // (unrolled: the operands of a K step are named registers)
#pragma unroll
                for (int k0 = 0; k0 < NB; k0 += MF::KT) kstep(k0);
            } else {
#pragma unroll 2
                for (int k0 = 0; k0 < NB; k0 += MF::KT) kstep(k0);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < MF::NREG; ++r) {
                    const int i = bi + 16 * a + MF::d_row(lane, r);
                    if (i >= r1 || (i >= kb && i < kb + nb)) continue;
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int j = bj + 16 * q + MF::d_col(lane);
                        if (j < n && !(j >= kb && j < kb + nb)) out(i, j, t.acc[a][q][r]);
                    }
                }
        };
        if (have0) tile_finish(bi0, bj0, t0);
        for (int blk = wave + SWEEP_THREADS / 64; blk < nrow * ncol; blk += SWEEP_THREADS / 64) {
            int bi, bj;
            if (!tile_at(blk, bi, bj)) continue;
            Tile t;
            tile_load(bi, bj, t);
            tile_finish(bi, bj, t);
        }
    }
    SKF_STAMP(3)
    // ---- the pivot columns of the slab's rows <- T, the pivot rows at the slab's columns <- T^T, the pivot block <- -P
    for (int i = r0 + ty; i < r1; i += 16) {
        if (tx >= nb) continue;
        if (i >= kb && i < kb + nb) out(i, kb + tx, Pv[(i - kb) * LD + tx]);
        else out(i, kb + tx, Ts[trow(i) * LD + tx]);
    }
    for (int idx = tid; idx < nb * (r1 - r0); idx += SWEEP_THREADS) {
        const int c = idx / (r1 - r0), i = r0 + idx % (r1 - r0);
        if (!(i >= kb && i < kb + nb)) out(kb + c, i, Ts[trow(i) * LD + c]);
    }
    SKF_STAMP(4)
#ifdef SKF_PROBE_STAMPS
    if (tid == 0 && n >= 200 && blockIdx.y == 1 && (step == 0 || step == 3))
        printf("sweep_step n %d step %d: loads + panel %lld, pivot block sweep %lld, T %lld, update %lld, write-back %lld (x10 ns)\n", n, step,
               ph[0], ph[1], ph[2], ph[3], ph[4]);
#endif
    if (tid == 0 && blockIdx.y == 0) e.chol_ok[b] = last ? 1 : SWEEP_RUNNING;
}

// K(r,c) = sum_k Vs(r,k) * V(c,k), r,c < n  (tiny c x c product, f64 accumulate, cast to T)
template <typename T>
__global__ __launch_bounds__(256) void eigh_unpack_pinv_kernel(PinvBatch pb, const double* __restrict__ VsAll,
                                                               const double* __restrict__ VAll, int64_t stride,
                                                               const int* __restrict__ chol_ok) {
    const int b = blockIdx.y;
    if (chol_ok[b] == 1) return;
    const int n = pb.c[b], n_pad = pb.n_pad[b];
    const double* Vs = VsAll + (int64_t)b * stride;
    const double* V = VAll + (int64_t)b * stride;
    T* K = (T*)pb.K[b];
    const int64_t ldk = pb.ldk[b];
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n * n; idx += gridDim.x * blockDim.x) {
        const int r = idx / n, c = idx % n;
        double s = 0.0;
        for (int k = 0; k < n_pad; ++k) s += Vs[r * n_pad + k] * V[c * n_pad + k];
        K[(int64_t)r * ldk + c] = (T)s;
    }
}

}  // namespace skf
