// skf_complete.h -- the consuming side of a completion model, never densified: the k best columns of every row and the
// predictions at given (row, column) pairs of X = G_row S G_col^T.
//
// The reference materialises X on the host (fusion/base/base.py `complete`: np.dot(G1, np.dot(S, G2.T))) and its users index or
// rank that array (examples/movielens_completion.py:121-126 evaluates R12_pred[hidden]).  Both kernels here work on
//     H = G_row[rows] S        (m x c, formed by the caller with skf_gemm)      and      Gc = G_col   (n_cols x c)
// and never write a score tile to HBM.
//
// complete_topk_kernel: a workgroup owns 64 rows and a contiguous range of columns (blockIdx.y = the column split), walks the
// range in 64-column tiles in increasing order, forms each 64 x 64 score tile on the matrix cores (K loop over c in chunks of
// TOPK_KC, both operands staged per chunk) and selects on the CU.  score(r, j) is the SAME chain of 16x16x4 matrix
// instructions over k = 0, 4, 8, ... whatever the tile position, the split count or the launch geometry (the K tail is zero
// filled on both sides: + 0 * 0), so the result does not depend on any of them, bit for bit.
//
// TOTAL ORDER of the selection: higher score first, equal scores by lower column index; a NaN score is never selected.
// Columns are visited in ascending order inside a split, so a score enters a row's list only when it is STRICTLY greater
// than the current k-th best (an equal score further right loses the tie), and is inserted behind every entry that is
// greater or equal.  The splits cover ascending, disjoint column ranges: the merge takes the heads in split order with a
// strict comparison, which is the same rule.  No float atomics anywhere.
#pragma once
#include "skf_kernels.h"

#include <cmath>

namespace skf {

constexpr int SKF_TOPK_MAX_K = 64;         // == SKF_TOPK_MAX of include/skfusion_hip.h (checked in skf_api.hip)
constexpr int TOPK_MAX_SPLITS = 32;        // column splits of one launch (the merge keeps one cursor per split in registers)
constexpr int TOPK_BM = 64, TOPK_BN = 64;  // score tile
constexpr int TOPK_KC = 32;                // K chunk staged per step
// operand tiles in LDS: row-major [64][TOPK_LD].  The A / B fragment of the 16x16x4 instructions reads (row = lane & 15,
// k = lane >> 4): with 34 elements per row a group of 32 lanes covers 32 distinct banks with ds_read_b32 (34 r + k mod 32
// = 2 r + k, k in {0, 1}) and 64 distinct banks with ds_read_b64 (68 r + 2 k mod 64 = 4 r + 2 k) -- no conflict either way.
constexpr int TOPK_LD = TOPK_KC + 2;
constexpr int TOPK_SLD = TOPK_BN + 1;      // score tile [64][65]: the selection reads it one row per lane
constexpr int TOPK_THREADS = 256;

// v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]; the accumulator
// register r of lane l holds D[row][l & 15], row = 4 (l >> 4) + r (f32) or (l >> 4) + 4 r (f64)
template <typename T> struct TopkMma;
template <> struct TopkMma<float> {
    typedef f32x4 acc_t;
    static __device__ __forceinline__ int d_row(int lane, int r) { return 4 * (lane >> 4) + r; }
    static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};
template <> struct TopkMma<double> {
    typedef f64x4 acc_t;
    static __device__ __forceinline__ int d_row(int lane, int r) { return (lane >> 4) + 4 * r; }
    static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
};

template <typename T>
struct TopkArgs {
    const T* H;  int64_t ldh;  int64_t m;           // [m][c]
    const T* Gc; int64_t ldg;  int64_t n_cols;      // [n_cols][c]
    int c, k;
    const int64_t* xptr; const int* xidx;           // exclusion CSR over the m rows (validated by the caller), or both null
    int tiles_per_split;                            // column tiles (of TOPK_BN) a split walks
    // splits == 1: the final lists; else the partial lists of split s at ((s * m + row) * k) of part_idx / part_val
    int* out_idx; int64_t ld_idx; T* out_val; int64_t ld_val;
    int* part_idx; T* part_val;
};

// bytes of dynamic LDS: the 64 running lists (values, then indices)
static inline size_t topk_list_bytes(int k, size_t esz) { return (size_t)TOPK_BM * k * (esz + sizeof(int)); }

template <typename T>
__global__ __launch_bounds__(TOPK_THREADS) void complete_topk_kernel(TopkArgs<T> a) {
    typedef TopkMma<T> M;
    // the operand tiles of a K chunk and the finished score tile share one buffer (a barrier on either side of the hand-over)
    constexpr int OPER = 2 * TOPK_BM * TOPK_LD, TILE = TOPK_BM * TOPK_SLD;
    __shared__ T buf[OPER > TILE ? OPER : TILE];
    __shared__ unsigned short cmask[4 * TOPK_BM];       // [column quarter][row]: the columns of the tile that pass the row's threshold
    __shared__ int cnt[TOPK_BM];                        // entries in the row's list
    HIP_DYNAMIC_SHARED(double, dyn)                     // lv[64][k] (T), then li[64][k] (int)
    T* lv = (T*)dyn;
    int* li = (int*)(lv + (size_t)TOPK_BM * a.k);
    T* sH = buf;
    T* sG = buf + TOPK_BM * TOPK_LD;
    T* sc = buf;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1;            // 2 x 2 waves, 32 x 32 scores each (2 x 2 instruction tiles)
    const int k = a.k, c = a.c;
    const int64_t row0 = (int64_t)blockIdx.x * TOPK_BM;
    const int64_t ntiles = (a.n_cols + TOPK_BN - 1) / TOPK_BN;
    const int64_t tile_lo = (int64_t)blockIdx.y * a.tiles_per_split;
    const int64_t tile_hi = tile_lo + a.tiles_per_split < ntiles ? tile_lo + a.tiles_per_split : ntiles;

    // the owner of row r of the tile is lane (r & 15) of wave (r >> 4): the insertions of a tile run on all four SIMDs
    const bool owner = lane < 16;
    const int orow = wave * 16 + lane;
    const bool live = owner && row0 + orow < a.m;
    int64_t xp = 0, xe = 0;                              // cursor into the row's exclusion list (ascending, as the tiles are)
    if (live && a.xptr) {
        xp = a.xptr[row0 + orow];
        xe = a.xptr[row0 + orow + 1];
        const int64_t first = tile_lo * TOPK_BN;
        if (first > 0) {                                 // a later split starts at its first column: lower bound
            int64_t lo = xp, hi = xe;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if ((int64_t)a.xidx[mid] < first) lo = mid + 1; else hi = mid;
            }
            xp = lo;
        }
    }
    if (t < TOPK_BM) cnt[t] = 0;

    for (int64_t tile = tile_lo; tile < tile_hi; ++tile) {
        const int64_t col0 = tile * TOPK_BN;
        typename M::acc_t acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = typename M::acc_t{0, 0, 0, 0};

        for (int k0 = 0; k0 < c; k0 += TOPK_KC) {
            __syncthreads();                             // the previous chunk / the previous tile's selection has left `buf`
            // element e = t + 256 i: 32 adjacent lanes read 32 adjacent k of one row (whole 128 / 256 B segments) and write
            // 32 adjacent LDS words; rows / columns past the end and the K tail are zero
            T hv[8], gv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = t + TOPK_THREADS * i, r = e >> 5, kk = e & 31;
                const bool kin = k0 + kk < c;
                hv[i] = (kin && row0 + r < a.m) ? a.H[(row0 + r) * a.ldh + k0 + kk] : (T)0;
                gv[i] = (kin && col0 + r < a.n_cols) ? a.Gc[(col0 + r) * a.ldg + k0 + kk] : (T)0;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = t + TOPK_THREADS * i, r = e >> 5, kk = e & 31;
                sH[r * TOPK_LD + kk] = hv[i];
                sG[r * TOPK_LD + kk] = gv[i];
            }
            __syncthreads();
            const int left = c - k0;
            const int kend = left >= TOPK_KC ? TOPK_KC : (left + 3) / 4 * 4;
            const T* pa = sH + (wr * 32 + (lane & 15)) * TOPK_LD + (lane >> 4);
            const T* pb = sG + (wc * 32 + (lane & 15)) * TOPK_LD + (lane >> 4);
            for (int kk = 0; kk < kend; kk += 4) {
                const T a0 = pa[kk], a1 = pa[16 * TOPK_LD + kk];
                const T b0 = pb[kk], b1 = pb[16 * TOPK_LD + kk];
                acc[0][0] = M::mma(a0, b0, acc[0][0]);
                acc[0][1] = M::mma(a0, b1, acc[0][1]);
                acc[1][0] = M::mma(a1, b0, acc[1][0]);
                acc[1][1] = M::mma(a1, b1, acc[1][1]);
            }
        }
        __syncthreads();                                 // every wave is through with the operand tiles
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    sc[(wr * 32 + 16 * i + M::d_row(lane, r)) * TOPK_SLD + wc * 32 + 16 * j + (lane & 15)] = acc[i][j][r];
        __syncthreads();

        // all 256 threads: 16 scores of one row each against the row's threshold as it stands (it only rises: the owner
        // looks again before it inserts)
        {
            const int r = t & 63, q = t >> 6, n = cnt[r];
            const bool full = n == k;
            const T thr = full ? lv[r * k + k - 1] : (T)0;
            unsigned mk = 0;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const T s = sc[r * TOPK_SLD + q * 16 + b];
                const bool in = col0 + q * 16 + b < a.n_cols;
                if (in && (full ? s > thr : s == s)) mk |= 1u << b;
            }
            cmask[q * TOPK_BM + r] = (unsigned short)mk;
        }
        __syncthreads();

        if (live) {
            int n = cnt[orow];
            T* v = lv + orow * k;
            int* ix = li + orow * k;
            for (int q = 0; q < 4; ++q) {
                unsigned mk = cmask[q * TOPK_BM + orow];
                while (mk) {
                    const int b = __ffs((int)mk) - 1;
                    mk &= mk - 1;
                    const int j = q * 16 + b;
                    const T s = sc[orow * TOPK_SLD + j];
                    if (n == k && !(s > v[k - 1])) continue;
                    const int64_t col = col0 + j;
                    if (a.xptr) {
                        while (xp < xe && (int64_t)a.xidx[xp] < col) ++xp;
                        if (xp < xe && (int64_t)a.xidx[xp] == col) continue;
                    }
                    int p = n < k ? n : k - 1;
                    while (p > 0 && v[p - 1] < s) {
                        v[p] = v[p - 1];
                        ix[p] = ix[p - 1];
                        --p;
                    }
                    v[p] = s;
                    ix[p] = (int)col;
                    if (n < k) ++n;
                }
            }
            cnt[orow] = n;
        }
        // (the barrier at the top of the next tile's first chunk separates this selection from the next staging)
    }
    __syncthreads();

    // the lists, best first; slots no candidate filled: index -1, score -inf
    const bool parts = gridDim.y > 1;
    for (int e = t; e < TOPK_BM * k; e += TOPK_THREADS) {
        const int r = e / k, s = e - r * k;
        const int64_t row = row0 + r;
        if (row >= a.m) continue;
        const bool have = s < cnt[r];
        const int id = have ? li[r * k + s] : -1;
        const T val = have ? lv[r * k + s] : (T)(-INFINITY);
        if (parts) {
            const int64_t at = ((int64_t)blockIdx.y * a.m + row) * k + s;
            a.part_idx[at] = id;
            a.part_val[at] = val;
        } else {
            a.out_idx[row * a.ld_idx + s] = id;
            a.out_val[row * a.ld_val + s] = val;
        }
    }
}

// One thread per row: the k best of the `splits` partial lists under the same total order.  Every partial list is sorted
// and the splits hold ascending, disjoint column ranges, so among equal heads the first split has the lowest column.
template <typename T>
__global__ __launch_bounds__(256) void complete_topk_merge_kernel(const int* __restrict__ part_idx, const T* __restrict__ part_val, int64_t m,
                                                                  int k, int splits, int* __restrict__ out_idx, int64_t ld_idx,
                                                                  T* __restrict__ out_val, int64_t ld_val) {
    for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < m; row += (int64_t)gridDim.x * blockDim.x) {
        unsigned char pos[TOPK_MAX_SPLITS];
        for (int s = 0; s < TOPK_MAX_SPLITS; ++s) pos[s] = 0;
        for (int slot = 0; slot < k; ++slot) {
            int best = -1, bi = -1;
            T bv = (T)(-INFINITY);
            for (int s = 0; s < splits; ++s) {
                if (pos[s] >= k) continue;
                const int64_t at = ((int64_t)s * m + row) * k + pos[s];
                const int id = part_idx[at];
                if (id < 0) continue;                    // this split's list is exhausted
                const T v = part_val[at];
                if (best < 0 || v > bv) {
                    best = s;
                    bi = id;
                    bv = v;
                }
            }
            if (best >= 0) ++pos[best];
            out_idx[row * ld_idx + slot] = bi;
            out_val[row * ld_val + slot] = bv;
        }
    }
}

// bad[0] = 1 when an entry names a row outside [0, m) or a column outside [0, n_cols)
static __global__ __launch_bounds__(256) void complete_entries_check_kernel(const int* __restrict__ rows, const int* __restrict__ cols, int64_t n,
                                                                            int64_t m, int64_t n_cols, int* __restrict__ bad) {
    int off = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int r = rows[e], c = cols[e];
        if (r < 0 || (int64_t)r >= m || c < 0 || (int64_t)c >= n_cols) off = 1;
    }
    if (off) *bad = 1;
}

// out[e] = <H[rows[e]], Gc[cols[e]]>.  16 adjacent lanes share an entry: lane g reads columns g, g + 16, ... of the two
// gathered rows (adjacent lanes, adjacent columns) and adds them up in that order; the 16 partial sums then fold in a
// fixed xor tree (8, 4, 2, 1) -- two runs give the same bits.
constexpr int ENTRY_LANES = 16;
template <typename T>
__global__ __launch_bounds__(256) void complete_entries_kernel(const T* __restrict__ H, int64_t ldh, const T* __restrict__ Gc, int64_t ldg, int c,
                                                               const int* __restrict__ rows, const int* __restrict__ cols, int64_t n,
                                                               T* __restrict__ out) {
    constexpr int PER_WAVE = 64 / ENTRY_LANES;
    const int lane = threadIdx.x & 63, g = lane & (ENTRY_LANES - 1), sub = lane / ENTRY_LANES;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t e0 = wave * PER_WAVE; e0 < n; e0 += nwaves * PER_WAVE) {      // (wave-uniform trip count: the shuffles below)
        const int64_t e = e0 + sub;
        T sum = 0;
        if (e < n) {
            const T* h = H + (int64_t)rows[e] * ldh;
            const T* gc = Gc + (int64_t)cols[e] * ldg;
            for (int q = g; q < c; q += ENTRY_LANES) sum += h[q] * gc[q];
        }
#pragma unroll
        for (int off = ENTRY_LANES / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, ENTRY_LANES);
        if (e < n && g == 0) out[e] = sum;
    }
}

}  // namespace skf
