// skf_complete.h -- the consuming side of a completion model, never densified: the k best columns of every row and the
// predictions at given (row, column) pairs of X = G_row S G_col^T.
//
// The reference materialises X on the host (fusion/base/base.py `complete`: np.dot(G1, np.dot(S, G2.T))) and its users index or
// rank that array (examples/movielens_completion.py:121-126 evaluates R12_pred[hidden]).  Both kernels here work on
//     H = G_row[rows] S        (m x c, formed by the caller with skf_gemm)      and      Gc = G_col   (n_cols x c)
// and never write a score tile to HBM.  Host side (every check, the split decision, the launches, the C entry points):
// skf_complete.inc.  What the passes over the score tiles share lives here once: the
// product (topk_score_tile), a split's tile range (split_tiles), the owner lane's exclusion cursor and its lower bound
// (excl_seek) and the 64-bit exclusion mask of a tile (excl_tile_mask).
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
//
// RANKS of held-out pairs (what Recall@k, MRR, NDCG and AUC need of the array the reference's users rank,
// examples/movielens_completion.py:121-126).  For a target (r, j) with s = score(r, j):
//     rank(r, j) = #{ j' in [0, n_cols), j' != j, j' not in row r's exclusion list, score(r, j') not NaN,
//                     score(r, j') > s  or  (score(r, j') == s and j' < j) }
// -- the 0-based position of j in the total order above.  A target with a NaN score gets -1; a target that is itself in the
// exclusion list is still ranked (exclusion removes competitors only).  score(r, j) is formed by topk_score_tile, the one
// product every pass here shares, hence
//   P1: if (r, j) is not excluded and rank(r, j) = p < k <= 64, complete_topk on the same inputs returns out_idx[r][p] == j
//       and out_val[r][p] with the bits of the rank pass's out_val; if p >= k, j is not in row r's list
// for every col_splits of either operator.
//
// ABOVE a threshold (link prediction: every pair the reference's dense product, fusion/base/base.py `complete`, holds at or
// above a cut-off).  For row r with threshold thr[r]:
//     above(r) = { j in [0, n_cols) : j not in row r's exclusion list, score(r, j) >= thr[r] }
// with the IEEE comparison (a NaN score or threshold selects nothing), as canonical CSR.  Same product, hence
//   P2: with thr[r] = the k-th value of complete_topk on the same inputs, row r's entries ordered by (value descending,
//       column ascending) begin with top-k's list, bit for bit, and every further entry equals thr[r].
//
// The n BEST pairs of the whole relation (link prediction: "the 10 000 most confident new pairs, over all rows") need a cut-off
// nobody knows in advance: the exact n-th largest score over every candidate -- a column inside the relation, not in the
// row's exclusion list, with a score that is not NaN.  complete_digits_kernel is one counting pass of a radix select for
// it: the histogram of one digit of an order-preserving integer key of the candidates under a key prefix (see there).  The
// caller walks the histograms from the top digit down (32 or 64 key bits in passes of at most 11) and holds, at the end,
// T = the n-th largest candidate score, g = the candidates > T and e = the candidates == T.  Same product, integer counts, hence
//   P3: skf_complete_above with thr[r] = T in every row returns exactly g + e entries on the same inputs, g of them > T and e
//       of them == T, with g < n <= g + e -- for every col_splits and every cut of the rows into blocks; for a single row
//       and n <= 64 the n best pairs are complete_topk's list, index for index and bit for bit.
//
// The k best columns of EVERY row for any k (Recall@100 / @1000, R-precision, candidate lists: far beyond top-k's 64 slots) are
// above(r) at the row's own k-th score.  complete_row_digits_kernel / complete_row_walk_kernel run the selection above once
// per row -- one histogram and one prefix per row, every pass and every walk enqueued on the stream, no host round trip -- and
// leave, for want[r] with n_r = min(want[r], candidates of row r) > 0: thr[r] = the n_r-th largest candidate score of the row,
// greater[r] = the candidates above it, equal[r] = the candidates equal to it, greater[r] < n_r <= greater[r] + equal[r]; for
// n_r == 0: NaN, 0, 0.  Same product, integer counts, hence
//   P4: skf_complete_above on the same inputs with thr = that device array returns exactly greater[r] + equal[r] entries in row
//       r, greater[r] of them above thr[r], for every col_splits of either operator and every cut of the rows into blocks; a
//       NaN threshold selects nothing.
//   P5: with want[r] = k <= 64, row r's P4 entries ordered by (value descending, column ascending) begin with
//       complete_topk's list for that k -- its first min(k, candidates) slots -- index for index and bit for bit.
//
// How the scores of a whole relation are DISTRIBUTED (link prediction is judged by it: the pairs above each of many cut-offs,
// precision / recall / false-positive rate against a gold standard, the micro-averaged ROC and PR curves and the AUROC the
// reference's users read from roc_auc_score on the dense product, examples/pharma_chaining.py:100) is one more walk:
// complete_hist_kernel bins every candidate score by VALUE against up to 2047 edges, bin(s) = #{ t : edges[t] <= s }, and in the
// same launch, with the same bits, the scores of given target pairs.  Same product, the comparison of above(), integer counts:
//   P6: for every t, the sum of hist[b] over b > t (the increments of one call) equals *n_found of skf_complete_above on the
//       same inputs with thr[r] = edges[t] in every row, for every col_splits of either operator and every cut of the rows
//       into blocks.
//   P7: a counted target e lands in bin #{ t : edges[t] <= v }, v the out_val[e] of the rank pass on the same inputs.
#pragma once
#include "skf_kernels.h"

#include <cmath>

namespace skf {

constexpr int SKF_TOPK_MAX_K = 64;         // == SKF_TOPK_MAX of include/skfusion_hip.h (checked in skf_complete.inc)
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

// ---- the walk over a split's column tiles, shared by the top-k, rank-count and above passes --------------------------------
// Values and references to the callers' own variables in and out, never the argument block, and `col_of` of a contiguous
// tile stays a lambda at its three calls: in these forms every kernel compiles to the instruction stream of the separate
// copies (a struct for the cursor, a named functor for `col_of`, by value or by reference, each changed all eight:
// profiles/r21_complete_refactor.txt).
// the column tiles [lo, hi) of split blockIdx.y
struct TileRange { int64_t lo, hi; };
static __device__ __forceinline__ TileRange split_tiles(int64_t n_cols, int tiles_per_split) {
    const int64_t ntiles = (n_cols + TOPK_BN - 1) / TOPK_BN;
    const int64_t lo = (int64_t)blockIdx.y * tiles_per_split;
    return TileRange{lo, lo + tiles_per_split < ntiles ? lo + tiles_per_split : ntiles};
}

// The owner lane's cursor into its row's exclusion list (ascending, as the tiles are): positions [at, end) of xidx, placed
// at the first entry >= `first`, the split's first column (a later split starts inside the list: lower bound).  The caller
// asks only for a live row of given lists; otherwise its cursor stays empty (0, 0).
static __device__ __forceinline__ void excl_seek(const int64_t* xptr, const int* xidx, int64_t row, int64_t first, int64_t& at, int64_t& end) {
    at = xptr[row];
    end = xptr[row + 1];
    if (first > 0) {
        int64_t lo = at, hi = end;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if ((int64_t)xidx[mid] < first) lo = mid + 1; else hi = mid;
        }
        at = lo;
    }
}

// bit b: column col0 + b of the tile is in the row's list; the cursor moves past the tile
static __device__ __forceinline__ unsigned long long excl_tile_mask(const int* xidx, int64_t& at, int64_t end, int64_t col0) {
    unsigned long long mk = 0;
    while (at < end && (int64_t)xidx[at] < col0 + TOPK_BN) {
        mk |= 1ull << ((int64_t)xidx[at] - col0);
        ++at;
    }
    return mk;
}

// The argument blocks of the three passes over the score tiles begin with the same operands under the same names -- H, ldh,
// m, Gc, ldg, n_cols, c, xptr, xidx, tiles_per_split -- which the host fills in ONE place (skf_complete.inc, fill_operands).
// They stay three flat structs: a shared base moves the pass's own fields behind the operands, and with the kernel
// arguments laid out differently the kernels no longer compile to the instruction stream they had.
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

// The 64 x 64 score tile of rows row0 .. row0 + 63 of H against 64 rows of Gc, into sc = buf as [64][TOPK_SLD]: the K loop
// over c in chunks of TOPK_KC (both operands staged per chunk into buf as [64][TOPK_LD] each), the four chains of 16x16x4
// matrix instructions of every wave (2 x 2 waves, 32 x 32 scores each) and the hand-over of the accumulators, with a
// barrier on either side of it.  `col_of(r)`, r < 64, names the row of Gc that is column r of the tile, or -1 for none (its
// scores are 0): a contiguous tile and a gathered one run the SAME instructions on the same operands, so score(r, j) has the
// same bits wherever column j sits in whichever tile.  Every thread of the workgroup calls it; `buf` may still be read by
// the previous user on entry (the first barrier waits for it) and holds the finished tile, visible to all, on return.  What
// `col_of` reads must be in place before the call: it is asked ahead of that barrier.
template <typename T, class ColOf>
__device__ __forceinline__ void topk_score_tile(const T* __restrict__ H, int64_t ldh, int64_t m, int64_t row0, const T* __restrict__ Gc,
                                                int64_t ldg, int c, ColOf col_of, T* buf) {
    typedef TopkMma<T> M;
    T* sH = buf;
    T* sG = buf + TOPK_BM * TOPK_LD;
    T* sc = buf;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1;            // 2 x 2 waves, 32 x 32 scores each (2 x 2 instruction tiles)
    typename M::acc_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = typename M::acc_t{0, 0, 0, 0};
    int gcol[8];                                         // the rows of Gc this thread stages (the same for every chunk)
#pragma unroll
    for (int i = 0; i < 8; ++i) gcol[i] = col_of((t + TOPK_THREADS * i) >> 5);

    for (int k0 = 0; k0 < c; k0 += TOPK_KC) {
        __syncthreads();                                 // the previous chunk / the previous user has left `buf`
        // element e = t + 256 i: 32 adjacent lanes read 32 adjacent k of one row (whole 128 / 256 B segments) and write
        // 32 adjacent LDS words; rows / columns past the end and the K tail are zero
        T hv[8], gv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = t + TOPK_THREADS * i, r = e >> 5, kk = e & 31;
            const bool kin = k0 + kk < c;
            hv[i] = (kin && row0 + r < m) ? H[(row0 + r) * ldh + k0 + kk] : (T)0;
            gv[i] = (kin && gcol[i] >= 0) ? Gc[(int64_t)gcol[i] * ldg + k0 + kk] : (T)0;
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
    __syncthreads();                                     // every wave is through with the operand tiles
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                sc[(wr * 32 + 16 * i + M::d_row(lane, r)) * TOPK_SLD + wc * 32 + 16 * j + (lane & 15)] = acc[i][j][r];
    __syncthreads();
}

// bytes of dynamic LDS: the 64 running lists (values, then indices)
static inline size_t topk_list_bytes(int k, size_t esz) { return (size_t)TOPK_BM * k * (esz + sizeof(int)); }

template <typename T>
__global__ __launch_bounds__(TOPK_THREADS) void complete_topk_kernel(TopkArgs<T> a) {
    // the operand tiles of a K chunk and the finished score tile share one buffer (a barrier on either side of the hand-over)
    constexpr int OPER = 2 * TOPK_BM * TOPK_LD, TILE = TOPK_BM * TOPK_SLD;
    __shared__ T buf[OPER > TILE ? OPER : TILE];
    __shared__ unsigned short cmask[4 * TOPK_BM];       // [column quarter][row]: the columns of the tile that pass the row's threshold
    __shared__ int cnt[TOPK_BM];                        // entries in the row's list
    HIP_DYNAMIC_SHARED(double, dyn)                     // lv[64][k] (T), then li[64][k] (int)
    T* lv = (T*)dyn;
    int* li = (int*)(lv + (size_t)TOPK_BM * a.k);
    T* sc = buf;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int k = a.k, c = a.c;
    const int64_t row0 = (int64_t)blockIdx.x * TOPK_BM;
    const TileRange tiles = split_tiles(a.n_cols, a.tiles_per_split);

    // the owner of row r of the tile is lane (r & 15) of wave (r >> 4): the insertions of a tile run on all four SIMDs
    const bool owner = lane < 16;
    const int orow = wave * 16 + lane;
    const bool live = owner && row0 + orow < a.m;
    int64_t xp = 0, xe = 0;                              // cursor into the row's exclusion list
    if (live && a.xptr) excl_seek(a.xptr, a.xidx, row0 + orow, tiles.lo * TOPK_BN, xp, xe);
    if (t < TOPK_BM) cnt[t] = 0;

    for (int64_t tile = tiles.lo; tile < tiles.hi; ++tile) {
        const int64_t col0 = tile * TOPK_BN;
        topk_score_tile<T>(a.H, a.ldh, a.m, row0, a.Gc, a.ldg, c,
                           [&](int r) { return col0 + r < a.n_cols ? (int)(col0 + r) : -1; }, buf);

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

// ---- ranks of given (row, column) pairs -------------------------------------------------------------------------------------
// rank(r, j) of the header comment is a COUNT, so it needs no list: the score pass writes score(r, j) of every target
// (the shared score tile on 64 gathered columns: the same chain as anywhere else) and the count pass walks the columns as
// the top-k pass does and counts, per target, the admissible columns that come before it in the total order.  Counts are
// integers: LDS counters per workgroup, one integer atomicAdd per (target, split) at the end -- the sum does not depend on
// the splits, the chunk grid or the order of arrival.
constexpr int RANK_CHUNK = 32;                 // targets of one row a workgroup of the count pass holds
// chunk arrays [64][33]: the compare loop reads entry i of row (lane & 63) in all lanes at once -- 33 r + i (words) and
// 66 r + 2 i (f64, ds_read_b64: 64 banks) are distinct banks over a group of 32 lanes
constexpr int RANK_CLD = RANK_CHUNK + 1;
constexpr int RANK_MAX_PARTS = 64;             // workgroups (and result words) of rank_longest_row_kernel

// part[b] = the longest row (indptr[r + 1] - indptr[r], capped to int) among the rows workgroup b strides over.  Plain
// loads of the m + 1 pointers: it may run on lists the check has not passed yet (the result is then not used).
static __global__ __launch_bounds__(256) void rank_longest_row_kernel(const int64_t* __restrict__ indptr, int64_t rows, int* __restrict__ part) {
    __shared__ int red[256];
    const int t = threadIdx.x;
    int64_t best = 0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + t; r < rows; r += (int64_t)gridDim.x * 256) {
        const int64_t d = indptr[r + 1] - indptr[r];
        if (d > best) best = d;
    }
    red[t] = best > 0x7fffffff ? 0x7fffffff : (int)best;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s && red[t + s] > red[t]) red[t] = red[t + s];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = red[0];
}

template <typename T>
struct RankArgs {
    const T* H;  int64_t ldh;  int64_t m;           // [m][c]
    const T* Gc; int64_t ldg;  int64_t n_cols;      // [n_cols][c]
    int c;
    const int64_t* tptr; const int* tidx;           // target CSR over the m rows (validated by the caller)
    const int64_t* xptr; const int* xidx;           // exclusion CSR over the m rows (validated by the caller), or both null
    int tiles_per_split;                            // column tiles (of TOPK_BN) a split walks
    int chunk_groups;                               // workgroups per (row tile, split): chunk z, z + chunk_groups, ... each
    int* out_rank;                                  // [n_targets]
    T* val;                                         // [n_targets]: score of every target (the caller's out_val, or workspace)
};

// bytes of dynamic LDS of the count pass: the chunk's scores, columns and counters.  With the operand / score buffer the
// f64 kernel holds 69 KB of LDS, the f32 kernel 43 KB.
static inline size_t rank_chunk_bytes(size_t esz) { return (size_t)TOPK_BM * RANK_CLD * (esz + 2 * sizeof(int)); }

// A workgroup owns 64 rows; their targets are the contiguous entries tptr[row0] .. tptr[row0 + 64].  64 consecutive
// entries at a time are the 64 gathered columns of a score tile; entry e of row r reads sc[r - row0][e - e0].
template <typename T>
__global__ __launch_bounds__(TOPK_THREADS) void complete_rank_scores_kernel(RankArgs<T> a) {
    constexpr int OPER = 2 * TOPK_BM * TOPK_LD, TILE = TOPK_BM * TOPK_SLD;
    __shared__ T buf[OPER > TILE ? OPER : TILE];
    __shared__ int64_t tp[TOPK_BM + 1];                  // the target pointers of the 64 rows (rows past m: empty)
    __shared__ int gc[TOPK_BN];                          // the gathered columns of the tile, -1: none
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * TOPK_BM;
    if (t <= TOPK_BM) tp[t] = a.tptr[row0 + t < a.m ? row0 + t : a.m];
    __syncthreads();
    const int64_t e_hi = tp[TOPK_BM];
    for (int64_t e0 = tp[0]; e0 < e_hi; e0 += TOPK_BN) {
        // (a thread that writes gc here has passed the barriers of the previous tile, which every thread passes after
        // it has asked col_of)
        if (t < TOPK_BN) gc[t] = e0 + t < e_hi ? a.tidx[e0 + t] : -1;
        __syncthreads();
        topk_score_tile<T>(a.H, a.ldh, a.m, row0, a.Gc, a.ldg, a.c, [&](int r) { return gc[r]; }, buf);
        if (t < TOPK_BN && e0 + t < e_hi) {
            const int64_t e = e0 + t;
            int lo = 0, hi = TOPK_BM;                    // the row of entry e: tp[lo] <= e < tp[hi], rows may be empty
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (tp[mid] <= e) lo = mid; else hi = mid;
            }
            const T s = buf[lo * TOPK_SLD + t];
            a.val[e] = s;
            a.out_rank[e] = s == s ? 0 : -1;
        }
    }
}

// grid (target chunk within 64-row tile, column split): chunk z holds targets 32 z .. 32 z + 31 of each of its rows -- scores,
// columns and counters in LDS -- and walks its split's column tiles in ascending order.  Per tile the owner lane of a row
// (as in the top-k pass) advances the row's exclusion cursor over the tile's columns and publishes them as a 64-bit mask;
// then thread (row = t & 63, quarter = t >> 6) holds its 16 scores -- NaN where the column is past the end or excluded,
// so that it compares false like a NaN score does -- and runs over the row's chunk targets with the predicate of the
// definition.  (Column j itself has the target's own bits and fails both halves of it.)
template <typename T>
__global__ __launch_bounds__(TOPK_THREADS) void complete_rank_count_kernel(RankArgs<T> a) {
    constexpr int OPER = 2 * TOPK_BM * TOPK_LD, TILE = TOPK_BM * TOPK_SLD;
    __shared__ T buf[OPER > TILE ? OPER : TILE];
    HIP_DYNAMIC_SHARED(double, dyn)                      // the chunk (rank_chunk_bytes): score (T),
    T* ts = (T*)dyn;
    int* tc = (int*)(ts + TOPK_BM * RANK_CLD);           // column
    int* tn = tc + TOPK_BM * RANK_CLD;                   // and count so far of target i of row r at [r][i]
    __shared__ unsigned long long xmask[TOPK_BM];        // the excluded columns of the tile, per row
    __shared__ int64_t tp[TOPK_BM + 1];
    __shared__ int nt[TOPK_BM];                          // targets of the row in this chunk
    const T* sc = buf;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // blockIdx.x = chunk group + chunk_groups * row tile: the chunks of one long row are consecutive workgroups, which the
    // hardware hands round its dies in turn; as a slower grid dimension they would lie a whole number of row tiles apart
    const int64_t row0 = (int64_t)(blockIdx.x / a.chunk_groups) * TOPK_BM;
    const int64_t ch0 = blockIdx.x % a.chunk_groups;
    const TileRange tiles = split_tiles(a.n_cols, a.tiles_per_split);

    // the chunks this row tile needs: those of its longest row.  A workgroup beyond them leaves before it touches a list.
    if (t <= TOPK_BM) tp[t] = a.tptr[row0 + t < a.m ? row0 + t : a.m];
    __syncthreads();
    int64_t longest = 0;
    for (int r = 0; r < TOPK_BM; ++r) longest = tp[r + 1] - tp[r] > longest ? tp[r + 1] - tp[r] : longest;
    const int64_t chunks = (longest + RANK_CHUNK - 1) / RANK_CHUNK;
    if (ch0 >= chunks) return;

    const bool owner = lane < 16;                        // of row wave * 16 + lane of the tile
    const int orow = wave * 16 + lane;
    int64_t xp0 = 0, xe = 0;                             // the row's exclusion list from the split's first column on
    if (owner && row0 + orow < a.m && a.xptr) excl_seek(a.xptr, a.xidx, row0 + orow, tiles.lo * TOPK_BN, xp0, xe);

    for (int64_t ch = ch0; ch < chunks; ch += a.chunk_groups) {
        __syncthreads();                                 // the previous chunk's flush has left nt / tn
        if (t < TOPK_BM) {
            int64_t n = tp[t + 1] - tp[t] - ch * RANK_CHUNK;
            nt[t] = (int)(n < 0 ? 0 : (n > RANK_CHUNK ? RANK_CHUNK : n));
        }
        __syncthreads();
        for (int i = t; i < TOPK_BM * RANK_CHUNK; i += TOPK_THREADS) {
            const int r = i / RANK_CHUNK, q = i % RANK_CHUNK;
            if (q < nt[r]) {
                const int64_t e = tp[r] + ch * RANK_CHUNK + q;
                ts[r * RANK_CLD + q] = a.val[e];
                tc[r * RANK_CLD + q] = a.tidx[e];
                tn[r * RANK_CLD + q] = 0;
            }
        }
        int64_t xp = xp0;
        for (int64_t tile = tiles.lo; tile < tiles.hi; ++tile) {
            const int64_t col0 = tile * TOPK_BN;
            topk_score_tile<T>(a.H, a.ldh, a.m, row0, a.Gc, a.ldg, a.c,
                               [&](int r) { return col0 + r < a.n_cols ? (int)(col0 + r) : -1; }, buf);
            if (owner) xmask[orow] = excl_tile_mask(a.xidx, xp, xe, col0);
            __syncthreads();                             // (covers the chunk arrays too, on the first tile)
            const int r = t & 63, q = t >> 6, n = nt[r];
            if (n > 0) {
                const unsigned xm = (unsigned)(xmask[r] >> (16 * q)) & 0xffffu;
                const int64_t cb = col0 + 16 * q;
                T sv[16];
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    sv[b] = (cb + b < a.n_cols && !((xm >> b) & 1u)) ? sc[r * TOPK_SLD + 16 * q + b] : (T)NAN;
                for (int i = 0; i < n; ++i) {
                    const T s = ts[r * RANK_CLD + i];
                    const int64_t d = (int64_t)tc[r * RANK_CLD + i] - cb;
                    const int jb = d < 0 ? 0 : (d > 16 ? 16 : (int)d);      // columns cb + b with b < jb lie left of the target
                    int cn = 0;
#pragma unroll
                    for (int b = 0; b < 16; ++b) cn += (int)((sv[b] > s) | ((sv[b] == s) & (b < jb)));
                    if (cn) atomicAdd(&tn[r * RANK_CLD + i], cn);
                }
            }
            // (the first barrier of the next tile's product separates this compare from the next tile and mask)
        }
        __syncthreads();
        for (int i = t; i < TOPK_BM * RANK_CHUNK; i += TOPK_THREADS) {
            const int r = i / RANK_CHUNK, q = i % RANK_CHUNK;
            if (q < nt[r] && tn[r * RANK_CLD + q] != 0) atomicAdd(&a.out_rank[tp[r] + ch * RANK_CHUNK + q], tn[r * RANK_CLD + q]);
        }
    }
}

// ---- every pair at or above a per-row threshold, as CSR -------------------------------------------------------------------------
// above(r) of the header comment has no size known in advance, so the pass runs twice over the same tiles: the count pass
// leaves one integer per (split, row), the scan turns them into out_indptr and into the start of every (row, split) run --
// row r's entries are those of split 0, then split 1, ..., each in ascending columns, i.e. ascending columns altogether
// whatever the split count -- and the fill pass walks the tiles again and writes every selected (column, score) to
//     start(r, split) + #{ selected columns of row r in this split left of it }.
// Positions are functions of the inputs alone: no atomics on them, the same bytes for every col_splits and every run.
template <typename T>
struct AboveArgs {
    const T* H;  int64_t ldh;  int64_t m;           // [m][c]
    const T* Gc; int64_t ldg;  int64_t n_cols;      // [n_cols][c]
    int c;
    const T* thr;                                   // [m]
    const int64_t* xptr; const int* xidx;           // exclusion CSR over the m rows (validated by the caller), or both null
    int tiles_per_split;                            // column tiles (of TOPK_BN) a split walks
    int64_t* work;                                  // [splits][m]: the counts (count pass writes), then the starts (fill pass reads)
    const int64_t* indptr;                          // [m + 1]: out_indptr (fill pass: where row r's last split ends)
    int* out_indices; T* out_values;                // fill pass; out_values may be null
};

// THE predicate, for thread (row r, quarter q) of a finished score tile: bit b of the result says that column
// col0 + 16 q + b is in above(r) -- inside the relation, not in the row's exclusion mask `xm` (bit b: that column) and
// with a score >= thr under the IEEE comparison, which is false for a NaN on either side.
template <typename T>
__device__ __forceinline__ unsigned above_quarter_mask(const T* sc, int r, int q, int64_t col0, int64_t n_cols, unsigned xm, T thr) {
    unsigned mk = 0;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        const T s = sc[r * TOPK_SLD + 16 * q + b];
        if (col0 + 16 * q + b < n_cols && !((xm >> b) & 1u) && s >= thr) mk |= 1u << b;
    }
    return mk;
}

// grid (64-row tile, column split) as complete_topk_kernel.  Per tile the owner lane of a row publishes the excluded columns
// of the tile as a 64-bit mask (as complete_rank_count_kernel does); thread (row = t & 63, quarter = t >> 6) then holds the
// 16-bit mask of above_quarter_mask.  FILL = false adds its popcount to a register and the four quarters meet in LDS at the
// end; FILL = true publishes the four masks of a row, so that every thread of the row knows the selected columns left of
// its own, and keeps the row's write cursor in a register (all four advance it by the same total).
template <typename T, bool FILL>
__global__ __launch_bounds__(TOPK_THREADS) void complete_above_kernel(AboveArgs<T> a) {
    constexpr int OPER = 2 * TOPK_BM * TOPK_LD, TILE = TOPK_BM * TOPK_SLD;
    __shared__ T buf[OPER > TILE ? OPER : TILE];
    __shared__ unsigned long long xmask[TOPK_BM];        // the excluded columns of the tile, per row
    __shared__ unsigned short qmask[4 * TOPK_BM];        // FILL: [quarter][row] the selected columns of the tile
    __shared__ int qcnt[4 * TOPK_BM];                    // count: [quarter][row] at the end; FILL: word 0 = any row has entries
    const T* sc = buf;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = t & 63, q = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * TOPK_BM;
    const TileRange tiles = split_tiles(a.n_cols, a.tiles_per_split);
    const bool rin = row0 + r < a.m;

    int64_t pos = 0, end = 0;                            // FILL: where the row's next entry goes, and where its run ends
    if (FILL) {
        // the run of (row, split) ends where the next split's starts, the last one where the row ends
        if (rin) {
            pos = a.work[(int64_t)blockIdx.y * a.m + row0 + r];
            end = blockIdx.y + 1 < gridDim.y ? a.work[(int64_t)(blockIdx.y + 1) * a.m + row0 + r] : a.indptr[row0 + r + 1];
        }
        if (t == 0) qcnt[0] = 0;
        __syncthreads();
        if (q == 0 && end > pos) qcnt[0] = 1;
        __syncthreads();
        if (!qcnt[0]) return;                            // nothing of these 64 rows lies in this split: no product
    }

    const bool owner = lane < 16;                        // of row wave * 16 + lane of the tile
    const int orow = wave * 16 + lane;
    int64_t xp = 0, xe = 0;                              // the row's exclusion list from the split's first column on
    if (owner && row0 + orow < a.m && a.xptr) excl_seek(a.xptr, a.xidx, row0 + orow, tiles.lo * TOPK_BN, xp, xe);
    const T thr = rin ? a.thr[row0 + r] : (T)NAN;        // (a row past the end selects nothing)
    int cnt = 0;

    for (int64_t tile = tiles.lo; tile < tiles.hi; ++tile) {
        const int64_t col0 = tile * TOPK_BN;
        topk_score_tile<T>(a.H, a.ldh, a.m, row0, a.Gc, a.ldg, a.c,
                           [&](int rr) { return col0 + rr < a.n_cols ? (int)(col0 + rr) : -1; }, buf);
        if (owner) xmask[orow] = excl_tile_mask(a.xidx, xp, xe, col0);
        __syncthreads();
        const unsigned xm = (unsigned)(xmask[r] >> (16 * q)) & 0xffffu;
        const unsigned mk = above_quarter_mask<T>(sc, r, q, col0, a.n_cols, xm, thr);
        if (!FILL) {
            cnt += __popc(mk);
        } else {
            qmask[q * TOPK_BM + r] = (unsigned short)mk;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const int n = __popc((unsigned)qmask[qq * TOPK_BM + r]);
                all += n;
                if (qq < q) before += n;
            }
            int64_t at = pos + before;
            unsigned left = mk;
            while (left) {
                const int b = __ffs((int)left) - 1;
                left &= left - 1;
                if (at < end) {                          // (always, the count pass ran the same predicate: a guard, not a rule)
                    a.out_indices[at] = (int)(col0 + 16 * q + b);
                    if (a.out_values) a.out_values[at] = sc[r * TOPK_SLD + 16 * q + b];
                }
                ++at;
            }
            pos += all;
        }
        // (the first barrier of the next tile's product separates these reads from the next tile and masks)
    }
    if (!FILL) {
        qcnt[q * TOPK_BM + r] = cnt;
        __syncthreads();
        if (q == 0 && rin)
            a.work[(int64_t)blockIdx.y * a.m + row0 + r] =
                (int64_t)qcnt[r] + qcnt[TOPK_BM + r] + qcnt[2 * TOPK_BM + r] + qcnt[3 * TOPK_BM + r];
    }
}

// The scan over the rows, in integers, three launches: every workgroup adds up the row totals of its chunk of rows
// (a multiple of 256, at most ABOVE_SCAN_PARTS chunks); one workgroup turns the chunk sums into chunk starts; every
// workgroup walks its chunk again, 256 rows at a time, and writes out_indptr[row] and, in place of the counts, the start of
// every (row, split) run.  out_indptr[m] is the total.
constexpr int ABOVE_SCAN_PARTS = 1024;

// all 256 threads: the sum of v over the workgroup's threads before this one (exclusive) and over all of them (`total`)
static __device__ __forceinline__ int64_t above_block_scan(int64_t v, int64_t* red, int64_t* total) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int64_t add = t >= off ? red[t - off] : 0;
        __syncthreads();
        red[t] += add;
        __syncthreads();
    }
    const int64_t incl = red[t];
    *total = red[255];
    __syncthreads();                                     // `red` is free again
    return incl - v;
}

static __global__ __launch_bounds__(256) void above_chunk_sums_kernel(const int64_t* __restrict__ work, int64_t m, int splits, int64_t chunk,
                                                                      int64_t* __restrict__ parts) {
    __shared__ int64_t red[256];
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < m ? lo + chunk : m;
    int64_t sum = 0;
    for (int64_t row = lo + threadIdx.x; row < hi; row += 256)
        for (int s = 0; s < splits; ++s) sum += work[(int64_t)s * m + row];
    int64_t total;
    above_block_scan(sum, red, &total);
    if (threadIdx.x == 0) parts[blockIdx.x] = total;
}

// one workgroup: parts[b] becomes the entries of the chunks before b; out_indptr[m] the total
static __global__ __launch_bounds__(256) void above_chunk_starts_kernel(int64_t* __restrict__ parts, int nparts, int64_t m,
                                                                        int64_t* __restrict__ out_indptr) {
    __shared__ int64_t red[256];
    constexpr int PER = ABOVE_SCAN_PARTS / 256;          // consecutive chunks of one thread
    const int t = threadIdx.x;
    int64_t v[PER], sum = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        v[i] = t * PER + i < nparts ? parts[t * PER + i] : 0;
        sum += v[i];
    }
    int64_t total;
    int64_t run = above_block_scan(sum, red, &total);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        if (t * PER + i < nparts) parts[t * PER + i] = run;
        run += v[i];
    }
    if (t == 0) out_indptr[m] = total;
}

static __global__ __launch_bounds__(256) void above_offsets_kernel(int64_t* __restrict__ work, int64_t m, int splits, int64_t chunk,
                                                                   const int64_t* __restrict__ parts, int64_t* __restrict__ out_indptr) {
    __shared__ int64_t red[256];
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < m ? lo + chunk : m;
    int64_t base = parts[blockIdx.x];
    for (int64_t row0 = lo; row0 < hi; row0 += 256) {    // (chunk is a multiple of 256: the trip count is the workgroup's)
        const int64_t row = row0 + threadIdx.x;
        int64_t sum = 0;
        if (row < hi)
            for (int s = 0; s < splits; ++s) sum += work[(int64_t)s * m + row];
        int64_t total;
        int64_t at = base + above_block_scan(sum, red, &total);
        if (row < hi) {
            out_indptr[row] = at;
            for (int s = 0; s < splits; ++s) {
                const int64_t n = work[(int64_t)s * m + row];
                work[(int64_t)s * m + row] = at;
                at += n;
            }
        }
        base += total;
    }
}

// ---- one digit of a radix select over every admissible score -------------------------------------------------------------------
// The n best pairs of the WHOLE relation need the n-th largest score over all rows, and that is a selection, not a sort: a
// few counting passes over the tiles the passes above walk, each of which histograms one digit of an order-preserving
// integer key of the scores whose higher digits equal the prefix found so far.
//     key(s): u = the bits of s + 0 as an unsigned integer of KEY_BITS (32 / 64); key = u ^ (sign(u) ? all ones : sign bit)
// so that key(a) < key(b) <=> a < b for a, b not NaN; -0.0 + 0 = +0.0: the two zeros share one key (no -0.0 comes out of
// accumulators that start at +0, the rule is stated all the same); +-inf are ordinary keys.  A CANDIDATE is a score whose
// column is inside the relation, not in the row's exclusion list, and that is not NaN.  The bit cast is a plain
// __builtin_memcpy: the host emulator runs this file too.
template <typename T> struct ScoreKey;
template <> struct ScoreKey<float> {
    typedef unsigned int key_t;
    static constexpr int BITS = 32;
};
template <> struct ScoreKey<double> {
    typedef unsigned long long key_t;
    static constexpr int BITS = 64;
};
template <typename T>
static __device__ __forceinline__ typename ScoreKey<T>::key_t score_key(T s) {
    typedef typename ScoreKey<T>::key_t K;
    const T z = s + (T)0;
    K u;
    __builtin_memcpy(&u, &z, sizeof u);
    const K sign = (K)1 << (ScoreKey<T>::BITS - 1);
    return u ^ ((u & sign) ? ~(K)0 : sign);
}

constexpr int DIGIT_MAX_BITS = 11;                   // 2048 uint32 bins in LDS: 8 KB beside the 35 KB buffer of the f64 kernel
// A workgroup sees at most 64 x 64 scores per tile, all of which may fall into ONE bin: after 2^19 tiles a bin holds at most
// 2^31 and is added to the caller's histogram and cleared, long before its 32 bits could wrap.  (A split walks up to
// 2^31 / 64 = 2^25 tiles.)
constexpr int64_t DIGIT_FLUSH_TILES = (int64_t)1 << 19;

template <typename T>
struct DigitArgs {
    const T* H;  int64_t ldh;  int64_t m;           // [m][c]
    const T* Gc; int64_t ldg;  int64_t n_cols;      // [n_cols][c]
    int c;
    const int64_t* xptr; const int* xidx;           // exclusion CSR over the m rows (validated by the caller), or both null
    int tiles_per_split;                            // column tiles (of TOPK_BN) a split walks
    unsigned long long prefix;                      // a candidate counts when the top prefix_bits of its key equal it
    int prefix_bits, digit_bits;                    // prefix_bits + digit_bits <= KEY_BITS, 1 <= digit_bits <= DIGIT_MAX_BITS
    unsigned long long* hist;                       // [1 << digit_bits], ADDED to
};

// all threads: the workgroup's non-zero bins go to the caller's histogram with integer atomics and are cleared
static __device__ __forceinline__ void digit_flush(unsigned* bins, int nbins, unsigned long long* hist) {
    __syncthreads();
    for (int d = threadIdx.x; d < nbins; d += TOPK_THREADS) {
        const unsigned n = bins[d];
        if (n) {
            atomicAdd(&hist[d], (unsigned long long)n);
            bins[d] = 0;
        }
    }
    __syncthreads();
}

// grid (64-row tile, column split) and walk as complete_above_kernel: the same product, hence the bits every other operator
// sees, and the exclusion mask published per tile by the owner lanes.  Thread (row = t & 63, quarter = t >> 6) then walks
// its 16 scores: a candidate under the prefix adds one to the LDS bin of its digit
//     (key >> (KEY_BITS - prefix_bits - digit_bits)) & (2^digit_bits - 1).
// Real scores share a handful of exponents -- in the first pass nearly every score of a tile meets in the same few words --
// so a thread MERGES RUNS: consecutive candidates with one digit become one atomicAdd of their count.  Counts are integers:
// the histogram does not depend on the splits, the launch geometry or the order of arrival.  No float atomics.
template <typename T>
__global__ __launch_bounds__(TOPK_THREADS) void complete_digits_kernel(DigitArgs<T> a) {
    typedef typename ScoreKey<T>::key_t K;
    constexpr int OPER = 2 * TOPK_BM * TOPK_LD, TILE = TOPK_BM * TOPK_SLD;
    __shared__ T buf[OPER > TILE ? OPER : TILE];
    __shared__ unsigned long long xmask[TOPK_BM];        // the excluded columns of the tile, per row
    __shared__ unsigned bins[1 << DIGIT_MAX_BITS];
    const T* sc = buf;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = t & 63, q = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * TOPK_BM;
    const TileRange tiles = split_tiles(a.n_cols, a.tiles_per_split);
    const bool rin = row0 + r < a.m;
    const int nbins = 1 << a.digit_bits;
    const int shift = ScoreKey<T>::BITS - a.prefix_bits - a.digit_bits;      // 0 .. KEY_BITS - 1
    const K dmask = (K)(nbins - 1), prefix = (K)a.prefix;

    for (int d = t; d < nbins; d += TOPK_THREADS) bins[d] = 0;
    __syncthreads();

    const bool owner = lane < 16;                        // of row wave * 16 + lane of the tile
    const int orow = wave * 16 + lane;
    int64_t xp = 0, xe = 0;                              // the row's exclusion list from the split's first column on
    if (owner && row0 + orow < a.m && a.xptr) excl_seek(a.xptr, a.xidx, row0 + orow, tiles.lo * TOPK_BN, xp, xe);

    for (int64_t tile = tiles.lo; tile < tiles.hi; ++tile) {
        const int64_t col0 = tile * TOPK_BN;
        topk_score_tile<T>(a.H, a.ldh, a.m, row0, a.Gc, a.ldg, a.c,
                           [&](int rr) { return col0 + rr < a.n_cols ? (int)(col0 + rr) : -1; }, buf);
        if (owner) xmask[orow] = excl_tile_mask(a.xidx, xp, xe, col0);
        __syncthreads();
        if (rin) {
            const unsigned xm = (unsigned)(xmask[r] >> (16 * q)) & 0xffffu;
            int run_d = 0, run_n = 0;                    // the run of equal digits so far
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const T s = sc[r * TOPK_SLD + 16 * q + b];
                const K v = score_key<T>(s) >> shift;    // the prefix and the digit; the prefix is 0 for prefix_bits == 0
                const int d = (int)(v & dmask);
                if (col0 + 16 * q + b < a.n_cols && !((xm >> b) & 1u) && s == s && (v >> a.digit_bits) == prefix) {
                    if (run_n && d != run_d) {
                        atomicAdd(&bins[run_d], (unsigned)run_n);
                        run_n = 0;
                    }
                    run_d = d;
                    ++run_n;
                }
            }
            if (run_n) atomicAdd(&bins[run_d], (unsigned)run_n);
        }
        if (((tile - tiles.lo + 1) & (DIGIT_FLUSH_TILES - 1)) == 0) digit_flush(bins, nbins, a.hist);
        // (the first barrier of the next tile's product separates these reads from the next tile and mask)
    }
    digit_flush(bins, nbins, a.hist);
}

// ---- the histogram of every candidate score BY VALUE, and of the scores of given pairs -------------------------------------------
// complete_digits_kernel bins by key bits; a curve over cut-offs needs bins by value: bin(s) = #{ t < n_edges : edges[t] <= s },
// 0 .. n_edges, for edges that do not descend (validated by the caller: hist_edges_check_kernel).  `<=` is the comparison of
// above_quarter_mask read from the other side, so the candidates of the bins above t are above() at thr = edges[t] (P6).
constexpr int HIST_MAX_EDGES = 2047;                 // with bin 0: 2048 uint32 bins, the histogram of an 11-bit digit

// The search descends a perfect binary tree of 2^steps - 1 nodes, steps = ceil(log2(n_edges + 1)), over the edges padded with
// NaN at the upper end (NaN <= s is false for every s: a padded entry is never passed, and the search needs no bound check).
// The table holds the tree in BREADTH-FIRST order, the root at [1] ([0] is not used): node k = 2^l + p, the p-th of level l,
// is entry ((2 p + 1) << (steps - 1 - l)) - 1 of the padded edges; the children of k are 2 k and 2 k + 1.  The sorted order
// would put the 2^l nodes of a level 2^(steps - l) words apart -- on ONE bank from the level on whose stride reaches the bank
// row, as many LDS cycles as the lanes hold distinct nodes; breadth first they are adjacent words, 32 nodes on 32 banks.
static inline int hist_steps(int n_edges) {
    int steps = 0;
    while ((1 << steps) < n_edges + 1) ++steps;
    return steps;
}
// bytes of dynamic LDS: the padded table (T, a whole number of 8-byte words), bins [n_edges + 1] and, with targets, theirs.
// At the maximum the f64 kernel holds 16 + 8 + 8 KB beside the 35 KB buffer and the mask words: 67 KB, two workgroups per CU;
// 16 edges in f32 cost 128 + 68 (+ 68) bytes.
static inline size_t hist_lds_bytes(int n_edges, bool targets, size_t esz) {
    const size_t table = (((size_t)1 << hist_steps(n_edges)) * esz + 7) / 8 * 8;
    return table + (targets ? 2 : 1) * (size_t)(n_edges + 1) * sizeof(unsigned);
}

// bad[0] = 1 when an edge is NaN or smaller than the one before it (IEEE <=; equal neighbours pass: an empty bin)
template <typename T>
__global__ __launch_bounds__(256) void hist_edges_check_kernel(const T* __restrict__ edges, int n_edges, int* __restrict__ bad) {
    int off = 0;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x)
        if (edges[e] != edges[e] || (e > 0 && !(edges[e - 1] <= edges[e]))) off = 1;
    if (off) *bad = 1;
}

template <typename T>
struct HistArgs {
    const T* H;  int64_t ldh;  int64_t m;           // [m][c]
    const T* Gc; int64_t ldg;  int64_t n_cols;      // [n_cols][c]
    int c;
    const int64_t* xptr; const int* xidx;           // exclusion CSR over the m rows (validated by the caller), or both null
    int tiles_per_split;                            // column tiles (of TOPK_BN) a split walks
    const int64_t* tptr; const int* tidx;           // target CSR over the m rows (validated by the caller), or both null
    const T* edges;                                 // [n_edges], none NaN, non-decreasing (validated by the caller)
    int n_edges, steps;                             // 1 <= n_edges <= HIST_MAX_EDGES; steps = hist_steps(n_edges)
    unsigned long long* hist;                       // [n_edges + 1], ADDED to
    unsigned long long* hist_tgt;                   // [n_edges + 1], ADDED to; null iff no targets
};

// grid (64-row tile, column split), walk, product, exclusion mask and candidate rule of complete_digits_kernel.  The edges are
// staged once per workgroup; thread (row = t & 63, quarter = t >> 6) then finds the bins of its 16 scores by a binary search
// of a fixed number of steps without a branch -- k = 1; steps times: k = 2 k + (table[k] <= s); bin = k - 2^steps, the
// edges passed on the way down -- all 16 searches side by side, so that every step issues 16 independent LDS reads (the
// first reads one address in all lanes: a broadcast).  Real scores of one tile row fall into few bins: a thread MERGES RUNS
// of equal consecutive bins into one LDS atomicAdd, as the digits kernel does.  With targets the owner lanes publish a second
// 64-bit mask per row and tile through a second cursor (the code of the exclusion cursor on the target lists); a candidate
// whose bit is set adds one to the second set of bins as well -- targets are few: no runs there.  A target that is excluded
// or scores NaN is no candidate and is counted nowhere.  Overflow: a workgroup sees at most 64 x 64 scores per tile, all of
// which may fall into ONE bin: after DIGIT_FLUSH_TILES = 2^19 tiles a bin holds at most 2^31 and is flushed and cleared, long
// before its 32 bits could wrap, and a target bin never holds more than the bin beside it.  (A split of that length has 2^25
// columns: no test reaches it, and none tries.)  Counts are integers: the histograms do not depend on the splits, the launch
// geometry or the order of arrival.  No float atomics, no atomics on positions.
template <typename T>
__global__ __launch_bounds__(TOPK_THREADS) void complete_hist_kernel(HistArgs<T> a) {
    constexpr int OPER = 2 * TOPK_BM * TOPK_LD, TILE = TOPK_BM * TOPK_SLD;
    __shared__ T buf[OPER > TILE ? OPER : TILE];
    __shared__ unsigned long long xmask[TOPK_BM];        // the excluded columns of the tile, per row
    __shared__ unsigned long long tmask[TOPK_BM];        // the target columns of the tile, per row
    HIP_DYNAMIC_SHARED(double, dyn)                      // hist_lds_bytes: the padded edges, the bins, the target bins
    const T* sc = buf;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = t & 63, q = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * TOPK_BM;
    const TileRange tiles = split_tiles(a.n_cols, a.tiles_per_split);
    const bool rin = row0 + r < a.m;
    const bool targets = a.tptr != nullptr;
    const int nbins = a.n_edges + 1, table = 1 << a.steps;
    T* ed = (T*)dyn;
    unsigned* bins = (unsigned*)((char*)dyn + ((size_t)table * sizeof(T) + 7) / 8 * 8);
    unsigned* tbins = bins + nbins;                      // (only with targets)

    for (int k = t; k < table; k += TOPK_THREADS) {
        const int l = k ? 31 - __builtin_clz((unsigned)k) : 0;          // the level of node k; k = 0 is no node
        const int e = (((2 * (k - (1 << l)) + 1) << (a.steps - 1 - l))) - 1;
        ed[k] = (k && e < a.n_edges) ? a.edges[e] : (T)NAN;
    }
    for (int d = t; d < nbins; d += TOPK_THREADS) bins[d] = 0;
    if (targets)
        for (int d = t; d < nbins; d += TOPK_THREADS) tbins[d] = 0;
    if (t < TOPK_BM) tmask[t] = 0;
    __syncthreads();

    const bool owner = lane < 16;                        // of row wave * 16 + lane of the tile
    const int orow = wave * 16 + lane;
    int64_t xp = 0, xe = 0;                              // the row's exclusion list from the split's first column on
    int64_t tp = 0, te = 0;                              // ... and its target list
    if (owner && row0 + orow < a.m && a.xptr) excl_seek(a.xptr, a.xidx, row0 + orow, tiles.lo * TOPK_BN, xp, xe);
    if (owner && row0 + orow < a.m && targets) excl_seek(a.tptr, a.tidx, row0 + orow, tiles.lo * TOPK_BN, tp, te);

    for (int64_t tile = tiles.lo; tile < tiles.hi; ++tile) {
        const int64_t col0 = tile * TOPK_BN;
        topk_score_tile<T>(a.H, a.ldh, a.m, row0, a.Gc, a.ldg, a.c,
                           [&](int rr) { return col0 + rr < a.n_cols ? (int)(col0 + rr) : -1; }, buf);
        if (owner) xmask[orow] = excl_tile_mask(a.xidx, xp, xe, col0);
        if (owner && targets) tmask[orow] = excl_tile_mask(a.tidx, tp, te, col0);
        __syncthreads();
        if (rin) {
            const unsigned xm = (unsigned)(xmask[r] >> (16 * q)) & 0xffffu;
            const unsigned tm = (unsigned)(tmask[r] >> (16 * q)) & 0xffffu;
            T sv[16];
            int at[16];
            unsigned ok = 0;                             // bit b: score b is a candidate
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                sv[b] = sc[r * TOPK_SLD + 16 * q + b];
                at[b] = 1;
                if (col0 + 16 * q + b < a.n_cols && !((xm >> b) & 1u) && sv[b] == sv[b]) ok |= 1u << b;
            }
            for (int step = 0; step < a.steps; ++step) {
#pragma unroll
                for (int b = 0; b < 16; ++b) at[b] = 2 * at[b] + (ed[at[b]] <= sv[b] ? 1 : 0);
            }
            int run_d = 0, run_n = 0;                    // the run of equal bins so far
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                if ((ok >> b) & 1u) {
                    const int d = at[b] - table;
                    if (run_n && d != run_d) {
                        atomicAdd(&bins[run_d], (unsigned)run_n);
                        run_n = 0;
                    }
                    run_d = d;
                    ++run_n;
                    if ((tm >> b) & 1u) atomicAdd(&tbins[d], 1u);
                }
            }
            if (run_n) atomicAdd(&bins[run_d], (unsigned)run_n);
        }
        if (((tile - tiles.lo + 1) & (DIGIT_FLUSH_TILES - 1)) == 0) {
            digit_flush(bins, nbins, a.hist);
            if (targets) digit_flush(tbins, nbins, a.hist_tgt);
        }
        // (the first barrier of the next tile's product separates these reads from the next tile and masks)
    }
    digit_flush(bins, nbins, a.hist);
    if (targets) digit_flush(tbins, nbins, a.hist_tgt);
}

// ---- the k best columns of EVERY row, for any k: one radix select per row, all passes on the device --------------------------
// complete_topk's lists end at 64 entries; beyond that a row's k best columns are above(r) at the row's own k-th score, and that
// score is the selection of complete_digits_kernel run per row: rows are independent, so the passes of a block of rows follow
// each other on the stream -- a counting pass (complete_row_digits_kernel), then one wave per row that reads the row's
// histogram and extends the row's prefix (complete_row_walk_kernel) -- with no host round trip, and the thresholds go to
// complete_above_kernel as a device pointer.  A digit has ROW_DIGIT_BITS bits (the last one what is left of the key):
//     width 8: 4 passes in f32, 8 in f64, 64 x 257 words of bins = 64.25 KB beside the 17 / 35 KB tile buffer: one workgroup per CU
//     width 7: 5 / 10 passes, 32.25 KB of bins: two to three workgroups per CU
// Both compile (-DSKF_ROW_DIGIT_BITS=8).  Measured on the MI355X (profiles/row_best.txt, one block of 8192 rows x 400 000
// columns): a pass at width 8 costs 1.6 to 1.8 times a pass at width 7 -- the lone workgroup per CU has nothing to hide its
// barriers and LDS atomics behind -- so the whole select is 1.27 to 1.46 times faster at width 7 in spite of its extra passes.
#ifndef SKF_ROW_DIGIT_BITS
#define SKF_ROW_DIGIT_BITS 7
#endif
constexpr int ROW_DIGIT_BITS = SKF_ROW_DIGIT_BITS;
static_assert(ROW_DIGIT_BITS >= 6 && ROW_DIGIT_BITS <= 8, "the walk gives every lane of a wave at least one bin; 64 rows of 2^9 bins do not fit the LDS");
constexpr int ROW_BINS = 1 << ROW_DIGIT_BITS;
// Real scores share a few exponents: in the first pass the 64 lanes of a wave -- 64 ROWS, one quarter -- mostly hold the same
// digit.  With a row stride of 2^D words they would all hit one bank; with 2^D + 1 lane r hits bank (r + d) mod 64.
constexpr int ROW_BIN_LD = ROW_BINS + 1;
static inline size_t row_bins_bytes() { return (size_t)TOPK_BM * ROW_BIN_LD * sizeof(unsigned); }

template <typename T>
struct RowDigitArgs {
    const T* H;  int64_t ldh;  int64_t m;           // [m][c]
    const T* Gc; int64_t ldg;  int64_t n_cols;      // [n_cols][c]
    int c;
    const int64_t* xptr; const int* xidx;           // exclusion CSR over the m rows (validated by the caller), or both null
    int tiles_per_split;                            // column tiles (of TOPK_BN) a split walks
    const unsigned long long* prefix;               // [m]: a candidate of row r counts when the top prefix_bits of its key equal prefix[r]
    const int64_t* need;                            // [m]: prefix_bits > 0 and need[r] == 0: the row has nothing to select, it is skipped
    int prefix_bits, digit_bits;                    // prefix_bits + digit_bits <= KEY_BITS, 1 <= digit_bits <= ROW_DIGIT_BITS
    unsigned* hist;                                 // [m][ROW_BINS], ADDED to (a row has < 2^31 columns: 32 bits cannot wrap)
};

// grid (64-row tile, column split), walk, product, exclusion mask and candidate rule of complete_digits_kernel; one histogram
// PER ROW in LDS (dynamic: [64][ROW_BIN_LD] words) and one prefix per row.  Thread (row = t & 63, quarter = t >> 6) walks its
// 16 scores and merges runs of equal digits into one LDS atomicAdd.  A workgroup sees at most 2^31 columns of a row: the
// bins need no intermediate flush.  At the end the non-zero bins are added to the row's histogram in the workspace with
// integer atomics: the counts do not depend on the splits, the launch geometry or the order of arrival.  No float atomics.
template <typename T>
__global__ __launch_bounds__(TOPK_THREADS) void complete_row_digits_kernel(RowDigitArgs<T> a) {
    typedef typename ScoreKey<T>::key_t K;
    constexpr int OPER = 2 * TOPK_BM * TOPK_LD, TILE = TOPK_BM * TOPK_SLD;
    __shared__ T buf[OPER > TILE ? OPER : TILE];
    __shared__ unsigned long long xmask[TOPK_BM];        // the excluded columns of the tile, per row
    __shared__ int any;                                  // a row of these 64 still selects
    HIP_DYNAMIC_SHARED(double, dyn)                      // bins[64][ROW_BIN_LD] (row_bins_bytes)
    unsigned* bins = (unsigned*)dyn;
    const T* sc = buf;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = t & 63, q = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * TOPK_BM;
    const TileRange tiles = split_tiles(a.n_cols, a.tiles_per_split);
    const bool rin = row0 + r < a.m && (a.prefix_bits == 0 || a.need[row0 + r] > 0);
    const int shift = ScoreKey<T>::BITS - a.prefix_bits - a.digit_bits;      // 0 .. KEY_BITS - 1
    const K dmask = (K)((1 << a.digit_bits) - 1);
    const K prefix = (rin && a.prefix_bits) ? (K)a.prefix[row0 + r] : (K)0;

    if (t == 0) any = 0;
    for (int i = t; i < TOPK_BM * ROW_BIN_LD; i += TOPK_THREADS) bins[i] = 0;
    __syncthreads();
    if (q == 0 && rin) any = 1;
    __syncthreads();
    if (!any) return;                                    // every row of the tile is through: no product

    const bool owner = lane < 16;                        // of row wave * 16 + lane of the tile
    const int orow = wave * 16 + lane;
    int64_t xp = 0, xe = 0;                              // the row's exclusion list from the split's first column on
    if (owner && row0 + orow < a.m && a.xptr) excl_seek(a.xptr, a.xidx, row0 + orow, tiles.lo * TOPK_BN, xp, xe);
    unsigned* mine = bins + r * ROW_BIN_LD;

    for (int64_t tile = tiles.lo; tile < tiles.hi; ++tile) {
        const int64_t col0 = tile * TOPK_BN;
        topk_score_tile<T>(a.H, a.ldh, a.m, row0, a.Gc, a.ldg, a.c,
                           [&](int rr) { return col0 + rr < a.n_cols ? (int)(col0 + rr) : -1; }, buf);
        if (owner) xmask[orow] = excl_tile_mask(a.xidx, xp, xe, col0);
        __syncthreads();
        if (rin) {
            const unsigned xm = (unsigned)(xmask[r] >> (16 * q)) & 0xffffu;
            int run_d = 0, run_n = 0;                    // the run of equal digits so far
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const T s = sc[r * TOPK_SLD + 16 * q + b];
                const K v = score_key<T>(s) >> shift;    // the prefix and the digit; the prefix is 0 for prefix_bits == 0
                const int d = (int)(v & dmask);
                if (col0 + 16 * q + b < a.n_cols && !((xm >> b) & 1u) && s == s && (v >> a.digit_bits) == prefix) {
                    if (run_n && d != run_d) {
                        atomicAdd(&mine[run_d], (unsigned)run_n);
                        run_n = 0;
                    }
                    run_d = d;
                    ++run_n;
                }
            }
            if (run_n) atomicAdd(&mine[run_d], (unsigned)run_n);
        }
        // (the first barrier of the next tile's product separates these reads from the next tile and mask)
    }
    __syncthreads();
    for (int i = t; i < TOPK_BM * ROW_BINS; i += TOPK_THREADS) {
        const int rr = i >> ROW_DIGIT_BITS, d = i & (ROW_BINS - 1);
        const unsigned n = bins[rr * ROW_BIN_LD + d];
        if (n && row0 + rr < a.m) atomicAdd(&a.hist[(row0 + rr) * ROW_BINS + d], n);
    }
}

// want[r] >= 0 for every row, or bad[0] = 2 (the list check beside it writes 1: whichever lands, the call is refused for a
// defect its message names)
static __global__ __launch_bounds__(256) void row_want_check_kernel(const int64_t* __restrict__ want, int64_t m, int* __restrict__ bad) {
    int off = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (int64_t)gridDim.x * blockDim.x)
        if (want[r] < 0) off = 1;
    if (off) *bad = 2;
}

struct RowWalkArgs {
    unsigned* hist;                                 // [m][ROW_BINS]: read, then cleared for the next pass
    int64_t m;
    int digit_bits;                                 // of the pass just counted
    int first, last;                                // first: no prefix yet, cands / need are set; last: the key is complete, thr is written
    const int64_t* want;                            // [m]
    unsigned long long* prefix;                     // [m]
    int64_t* need;                                  // [m]: the candidate wanted among those under the prefix, 1-based; 0: none
    int64_t* greater; int64_t* equal;               // [m]
    int64_t* cands;                                 // [m] or null
    void* thr;                                      // [m] of T
};

// One wave per row, after every counting pass: lane l holds bins ROW_BINS - 1 - PER l, ... downwards (PER = ROW_BINS / 64), so
// an inclusive scan over the lanes counts the candidates from the highest digit down.  The lane in which the running count
// reaches need[r] finds the bin; digit, the count above it and the bin's own count go round by shuffle.  Integers only: the
// result is a pure function of the histogram.  (The bins past 2^digit_bits of a short last digit are zero.)
template <typename T>
__global__ __launch_bounds__(256) void complete_row_walk_kernel(RowWalkArgs a) {
    typedef typename ScoreKey<T>::key_t K;
    constexpr int PER = ROW_BINS / 64;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t row = wave; row < a.m; row += nwaves) {                     // (wave-uniform: the shuffles below)
        unsigned* h = a.hist + row * ROW_BINS;
        int64_t cnt[PER], sum = 0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int d = ROW_BINS - 1 - (lane * PER + i);
            cnt[i] = (int64_t)h[d];
            h[d] = 0;
            sum += cnt[i];
        }
        int64_t incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t up = __shfl_up(incl, (unsigned)off);
            if (lane >= off) incl += up;
        }
        const int64_t total = __shfl(incl, 63);
        int64_t need = 0;
        if (a.first) {
            const int64_t w = a.want[row];
            need = w < total ? w : total;
        } else {
            need = a.need[row];
        }
        // the lane and the bin in which the count from the top reaches `need` (need <= total: the bin chosen before holds it)
        const int64_t before = incl - sum;
        int digit = 0;
        int64_t above = 0, eq = 0;
        const bool here = need > 0 && before < need && need <= incl;
        if (here) {
            int64_t ahead = before;
#pragma unroll
            for (int i = 0; i < PER; ++i) {                                  // (exactly one bin of the lane holds it)
                if (ahead < need && need <= ahead + cnt[i]) {
                    digit = ROW_BINS - 1 - (lane * PER + i);
                    above = ahead;
                    eq = cnt[i];
                }
                ahead += cnt[i];
            }
        }
        const unsigned long long who = __ballot(here);
        const int src = who ? __ffsll((long long)who) - 1 : 0;
        digit = __shfl(digit, src);
        above = __shfl(above, src);
        eq = __shfl(eq, src);
        if (lane == 0) {
            if (a.first && a.cands) a.cands[row] = total;
            if (need == 0) {                                                 // no candidate, or none wanted
                a.need[row] = 0;
                a.greater[row] = 0;
                a.equal[row] = 0;
                if (a.first) a.prefix[row] = 0;
                if (a.last) {
                    const T none = (T)NAN;
                    ((T*)a.thr)[row] = none;
                }
            } else {
                const K key = (a.first ? (K)0 : (K)a.prefix[row] << a.digit_bits) | (K)digit;
                a.prefix[row] = (unsigned long long)key;
                a.need[row] = need - above;
                a.greater[row] = (a.first ? 0 : a.greater[row]) + above;
                a.equal[row] = eq;
                if (a.last) {                                                // the score whose key this is; key(+0.0) -> +0.0
                    const K sign = (K)1 << (ScoreKey<T>::BITS - 1);
                    const K u = (key & sign) ? key ^ sign : ~key;
                    T s;
                    __builtin_memcpy(&s, &u, sizeof s);
                    ((T*)a.thr)[row] = s;
                }
            }
        }
    }
}

}  // namespace skf
