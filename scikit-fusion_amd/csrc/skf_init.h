// skf_init.h -- the column-mean initialisers `random_c` / `random_vcol` on the device (reference _init.py:20-61).
//
// The reference fills factor column k of an object type with the mean of `take` = int(0.2 m) randomly chosen columns of
// every relation that touches the type (oriented so that the type's objects are the rows: V, n x m), and `random_c` draws
// them from the half of the columns with the largest 2-norm:
//     G = 1e-5 + sum over the views of | V[:, chosen_k].mean(axis = 1) |          (_init.py:36-40, 56-60).
// With W (m x c) the 0/1 matrix of the chosen columns, the means are (V W) / take: one contraction of the relation in its
// stored form against a right operand that is exact in every type, bf16 included -- the product P = R G_j / Q = R^T G_i of
// the iteration with W in the place of the factor (relation_gemm, skf_plan.inc).  What lives here is everything around
// that product; the host side (checks, scratch layout, launches, C entry points) is skf_init.inc.
//
//   norms_*_kernel          one pass over a relation as stored -> the f64 sum of squares of every row and every column
//                           (`random_c` ranks the columns of a view by them; the host takes the square roots and sorts)
//   init_sel_check_kernel   an index of `sel` outside [0, m) raises the flag, before anything is written
//   init_sel_scatter_kernel W from `sel` (c x take int32, row k = the columns averaged into factor column k; the indices of
//                           one row are DISTINCT -- the caller's duty: two equal indices would count a column once, where the
//                           reference's mean counts it twice; the Python binding checks it): ones scattered into a zeroed
//                           buffer, either [m][c] in the master type or the bf16 Bt[c][Kp] layout of the bf16 contraction
//   init_acc_*              the f64 accumulator: starts at 1e-5, every view adds |x / (double)take| in view order, one
//                           rounding to the master type at the end -- the host's statement in the host's order, so that
//                           exact sums (0/1 data, small integers) give the reference's bits in every engine.
//   init_list_means_kernel, init_fill_colsum_kernel, norms_filled_kernel
//                           relations with MISSING values kept as lists (known entries over a constant; entries plus rank
//                           one): no product stands for V W there -- one pass over the view's lists against one-byte
//                           flags of the chosen columns, the fill beneath the unknown entries in the epilogue, added into
//                           the same accumulator; the line norms of the filled relation (statement further down)
// No atomics anywhere: every output element has one owner, every sum a fixed order.
#pragma once
#include "skf_known.h"

namespace skf {

constexpr int NORM_ROWS = 512;      // rows of a slab: one workgroup per (slab, 256 columns)
constexpr int NORM_COLS = 256;

// how a stored dense form yields the value at (r, c)
template <typename T>
struct NormDense {
    const T* R; int64_t ld;
    __device__ __forceinline__ double sq(int64_t r, int64_t c) const {
        const double v = (double)GatherT<T>::get(R[r * ld + c]);
        return v * v;
    }
};
// the bitmap of a SKF_REL_BINARY relation of the bf16 engine: bit (c & 7) of byte [r * ld + (c >> 3)]
struct NormBits {
    const uint8_t* B; int64_t ld;
    __device__ __forceinline__ double sq(int64_t r, int64_t c) const { return (double)((B[r * ld + (c >> 3)] >> (c & 7)) & 1); }
};

// Workgroup (blockIdx.x = slab, blockIdx.y = column block) walks its NORM_ROWS x NORM_COLS tile row by row, thread t on
// column t: the column's squares add up in a register in ascending row order -> colpart[slab][column]; the squares of a
// row meet in a butterfly over the wave (the same sum in every lane) and the four waves in LDS, first to last
// -> rowpart[column block][row].  norms_final sums the partials of a line first to last.  The grid follows from the
// shape alone and nothing is added atomically: the same bits on every run.
template <class Load>
__global__ __launch_bounds__(256) void norms_tile_kernel(Load ld, int64_t rows, int64_t cols, double* __restrict__ colpart,
                                                         double* __restrict__ rowpart) {
    __shared__ double wsum[4][NORM_ROWS];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t r0 = (int64_t)blockIdx.x * NORM_ROWS;
    const int64_t c = (int64_t)blockIdx.y * NORM_COLS + tid;
    const int nr = (int)(rows - r0 < NORM_ROWS ? rows - r0 : NORM_ROWS);
    double ca = 0.0;
    for (int i = 0; i < nr; ++i) {
        const double q = c < cols ? ld.sq(r0 + i, c) : 0.0;
        ca += q;
        double s = q;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        if (lane == 0) wsum[wave][i] = s;
    }
    __syncthreads();
    if (c < cols) colpart[(int64_t)blockIdx.x * cols + c] = ca;
    for (int i = tid; i < nr; i += 256)
        rowpart[(int64_t)blockIdx.y * rows + r0 + i] = ((wsum[0][i] + wsum[1][i]) + wsum[2][i]) + wsum[3][i];
}

// out[q] = part[0][q] + part[1][q] + ... (first to last), one thread per line
static __global__ __launch_bounds__(256) void norms_final_kernel(const double* __restrict__ part, int64_t nparts, int64_t n,
                                                                 double* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    double s = part[q];
    for (int64_t b = 1; b < nparts; ++b) s += part[b * n + q];
    out[q] = s;
}

// A relation kept as the lists of its stored entries (SKF_REL_SPARSE_CSR): line o owns the entries
// [ptr[o * parts], ptr[(o + 1) * parts]) of its list -- the row lists give the row sums, the column lists the column sums,
// each added in list order by the line's one thread (what is not stored is zero)
template <typename TM>
__global__ __launch_bounds__(256) void norms_lists_kernel(const int64_t* __restrict__ ptr, int parts, const TM* __restrict__ vals,
                                                          int64_t n, double* __restrict__ out) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n) return;
    double s = 0.0;
    for (int64_t e = ptr[o * parts]; e < ptr[(o + 1) * parts]; ++e) {
        const double v = (double)vals[e];
        s += v * v;
    }
    out[o] = s;
}

// bad[0] = 1 when one of the `total` indices lies outside [0, m)
static __global__ __launch_bounds__(256) void init_sel_check_kernel(const int* __restrict__ sel, int64_t total, int64_t m,
                                                                    int* __restrict__ bad) {
    int off = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int v = sel[e];
        if (v < 0 || (int64_t)v >= m) off = 1;
    }
    if (off) bad[0] = 1;
}

// W[sel[k][t] * s_col + k * s_k] = one, over a zeroed buffer (indices checked; distinct within a row of sel: no element is
// written twice).  Master layout [m][c]: s_col = c, s_k = 1; bf16 Bt[c][Kp]: s_col = 1, s_k = Kp.
template <typename T>
__global__ __launch_bounds__(256) void init_sel_scatter_kernel(const int* __restrict__ sel, int c, int take, T* __restrict__ W,
                                                               int64_t s_col, int64_t s_k, T one) {
    const int64_t total = (int64_t)c * take;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
        W[(int64_t)sel[e] * s_col + (e / take) * s_k] = one;
}

static __global__ __launch_bounds__(256) void init_acc_start_kernel(double* __restrict__ acc, int64_t total) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) acc[e] = 1e-5;
}

// acc += |x / take|  (x: the n x c product of one view, master type, leading dimension c)
template <typename T>
__global__ __launch_bounds__(256) void init_acc_add_kernel(double* __restrict__ acc, const T* __restrict__ x, int64_t total, double take) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
        acc[e] += fabs((double)x[e] / take);
}

// ---- relations with missing values: the known entries over a fill ------------------------------------------------------------
// Two stored forms hold the entries of a relation whose other entries are NOT zero (`_init._KnownView` on the host):
//   known   the lists of a masked relation (r.kn: from a mask or from the caller's CSR); every entry not stored holds the
//           constant f the caller passes (KnownEntries.fill)
//   rank1   SKF_REL_SPARSE_CSR | SKF_REL_FILL_RANK1: the lists hold d = v - a_r b_c, an entry not stored holds a_r b_c
// The product V W of such a view is not a contraction the plan runs (its list passes know nothing of what lies beneath the
// unknown entries), so the means come from a pass of their own over the lists.  V (n x m) is the oriented view, `own` the
// fill vector over its lines, `other` the one over its columns (a, b as the relation has them, or swapped for R^T):
//   known   mean_rk = (sum of the stored chosen v + (take - count_rk) f) / take
//           sq_c    = sum of the stored v^2 + (n - cnt_c) f^2
//   rank1   mean_rk = (sum of the stored chosen d + own_r B_k) / take,   B_k = sum of other over the chosen columns
//           sq_c    = sum over the stored of (d + own_r other_c)^2 + other_c^2 (|own|^2 - sum over the stored of own_r^2)
// (sq as norms_filled_kernel states it for the lines of the lists it walks: the column lists give the columns of R, the row
// lists its rows.)  Everything in f64, every sum in list order, one owner per output element.
//
// The epilogues are compiled with FP contraction OFF: (take - count) f + known and own_r B_k + sum d are each a product
// rounded, then a sum rounded, on the device as in a host model written with the same two operations -- the bound of the
// real-data tests has no term for a fused multiply-add, and exact data gives the same bits either way.

constexpr int INIT_FLAG_UNROLL = 4;     // entries of a line in flight per step of init_list_means_kernel

// B[k] = other[sel[k][0]] + other[sel[k][1]] + ... in the order of row k of sel, one thread per factor column
template <typename TM>
__global__ __launch_bounds__(256) void init_fill_colsum_kernel(const int* __restrict__ sel, int c, int take, const TM* __restrict__ other,
                                                               double* __restrict__ B) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= c) return;
    double s = 0.0;
    for (int t = 0; t < take; ++t) s += (double)other[sel[(int64_t)k * take + t]];
    B[k] = s;
}

// acc[r][k] += |mean_rk| for one view kept as lists over a fill.  A wave owns line r (256 threads: four lines per
// workgroup) and walks its entries [ptr[r * parts], ptr[(r + 1) * parts]) in list order -- the parts of a line are contiguous
// --, lane l owns the factor columns k = l + 64 j, j < NJ (NJ * 64 >= c: up to 16 sums and 16 counts in registers at rank
// 1024).  flags[col * c + k] != 0: column `col` of the view is averaged into factor column k -- the c flags of one entry are
// contiguous bytes, read coalesced by the wave.  The index and the value of an entry are wave-uniform loads; INIT_FLAG_UNROLL
// entries are loaded before the first of them is added, the adds stay in list order.  A long line (a popular item: tens
// of thousands of entries) runs serially in its wave, as the fold-in lists run theirs: DESIGN.md section 9.
// B == nullptr: the known form with the constant `fill`; else the rank-one form with own / B.
template <typename TM, int NJ>
__global__ __launch_bounds__(256) void init_list_means_kernel(const int64_t* __restrict__ ptr, int parts, const int* __restrict__ idx,
                                                              const TM* __restrict__ vals, const uint8_t* __restrict__ flags,
                                                              int64_t n, int c, int take, double fill, const TM* __restrict__ own,
                                                              const double* __restrict__ B, double* __restrict__ acc) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (r >= n) return;
    double sum[NJ];
    int cnt[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { sum[j] = 0.0; cnt[j] = 0; }
    const int64_t e0 = ptr[r * parts], e1 = ptr[(r + 1) * parts];
    int64_t e = e0;
    for (; e + INIT_FLAG_UNROLL <= e1; e += INIT_FLAG_UNROLL) {
        double v[INIT_FLAG_UNROLL];
        uint8_t f[INIT_FLAG_UNROLL][NJ];
#pragma unroll
        for (int u = 0; u < INIT_FLAG_UNROLL; ++u) {
            const uint8_t* row = flags + (int64_t)idx[e + u] * c;
            v[u] = (double)vals[e + u];
#pragma unroll
            for (int j = 0; j < NJ; ++j) f[u][j] = lane + 64 * j < c ? row[lane + 64 * j] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < INIT_FLAG_UNROLL; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (f[u][j]) { sum[j] += v[u]; ++cnt[j]; }
    }
    for (; e < e1; ++e) {
        const uint8_t* row = flags + (int64_t)idx[e] * c;
        const double v = (double)vals[e];
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (lane + 64 * j < c && row[lane + 64 * j]) { sum[j] += v; ++cnt[j]; }
    }
    const double a = B ? (double)own[r] : 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma clang fp contract(off)
        const int k = lane + 64 * j;
        if (k < c) {
            const double beneath = B ? a * B[k] : (double)(take - cnt[j]) * fill;
            const double mean = (sum[j] + beneath) / (double)take;
            acc[r * c + k] += fabs(mean);
        }
    }
}

// Sums of squares of the lines of one set of lists over a fill (see above): one thread per line o, its entries
// [ptr[o * parts], ptr[(o + 1) * parts]) in list order, no scratch.  n_other: the length of a line (the lines of the other
// orientation).  own == nullptr: the known form with the constant `fill`; else the rank-one form, own over these lines,
// other over what idx names, other_sq = |other|^2 (over every entry of `other`, stored against this line or not).
template <typename TM>
__global__ __launch_bounds__(256) void norms_filled_kernel(const int64_t* __restrict__ ptr, int parts, const int* __restrict__ idx,
                                                           const TM* __restrict__ vals, int64_t n, int64_t n_other, double fill,
                                                           const TM* __restrict__ own, const TM* __restrict__ other, double other_sq,
                                                           double* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n) return;
    const int64_t e0 = ptr[o * parts], e1 = ptr[(o + 1) * parts];
    double s = 0.0, so = 0.0;
    if (!own) {
        for (int64_t e = e0; e < e1; ++e) {
            const double v = (double)vals[e];
            const double q = v * v;
            s += q;
        }
        const double ff = fill * fill;
        const double beneath = (double)(n_other - (e1 - e0)) * ff;
        out[o] = s + beneath;
        return;
    }
    const double p = (double)own[o];
    for (int64_t e = e0; e < e1; ++e) {
        const double w = (double)other[idx[e]];
        const double pw = p * w;
        const double v = (double)vals[e] + pw;
        const double q = v * v;
        const double ww = w * w;
        s += q;
        so += ww;
    }
    const double pp = p * p;
    const double rest = other_sq - so;
    const double beneath = pp * rest;
    out[o] = s + beneath;
}

// G0[r][k] = (T)acc[r][k]; nothing past column c of a row is touched
template <typename T>
__global__ __launch_bounds__(256) void init_acc_store_kernel(const double* __restrict__ acc, int64_t n, int c, T* __restrict__ G0, int64_t ld) {
    const int64_t total = n * c;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
        G0[(e / c) * ld + e % c] = (T)acc[e];
}

}  // namespace skf
