// skf_heldout.h -- held-out pairs scored inside the fit: the squared error of a model on lists of (row, column, value)
// it never trained on, judged on the device after every iteration, and a device copy of the best (G, S).
//
// The reference stops a fit on its TRAINING objective (`stopping` / `stopping_system`, _dfmf.py:212-221, 301-322), which
// keeps falling while the model overfits.  The held-out error of a model is
//     sum over the list of (v - <(G_i S_ij)[r], G_j[c]>)^2
// -- the arithmetic of skf_complete_entries (skf_complete.h) on the plan's resident factors.  Host side (the checks, the
// workspace layout, the launches, the C entry points): skf_heldout.inc.
//
//   heldout_check_kernel     a list before anything gathers through it: rows in [0, n_i) and non-decreasing, columns in
//                            [0, n_j), values finite
//   heldout_sqerr_kernel     one f64 partial per slab of HELDOUT_SLAB = 1024 entries, fixed order (below), no atomics
//   heldout_judge_kernel     one workgroup: the partials of every list first to last, the history row, the pooled total and
//                            the monitor's state words
//   heldout_snapshot_kernel  every factor master and backbone into the snapshot, predicated on the device-side verdict
//
// H1: the prediction x of an entry has exactly the bits complete_entries_kernel returns on the same H and G_j: lane g of
// the 16 that share the entry adds h[q] * gc[q] over q = g, g + 16, ... in that order, and the 16 partial sums fold in the
// xor tree 8, 4, 2, 1 -- the same statements under the same contraction mode.  The residual is formed in f64,
// ((double)v - (double)x)^2, with FP contraction OFF (a difference rounded, then a product rounded: what a host model
// written with the same two operations gives, as in skf_init.h).
//
// ORDER of a slab's sum (what a host model restates): entry s of the slab (s < 1024; past the end of the list: +0.0)
// leaves its residual in res[s]; thread t forms a_t = ((res[t] + res[t + 256]) + res[t + 512]) + res[t + 768]; then for
// w = 128, 64, ..., 1: a_t += a_{t + w} for t < w; the partial is a_0.  A list's total is its partials added first to last.
#pragma once
#include "skf_kernels.h"
#include "skf_complete.h"

namespace skf {

constexpr int HELDOUT_SLAB = 1024;         // entries of one workgroup of the pass: the grid is fixed by n alone
constexpr int HELDOUT_THREADS = 256;

// The monitor's words on the device (the first 256 bytes of its workspace).  The host reads them between chunks of
// iterations and never to decide a launch.
struct HeldoutState {
    int64_t seen;          // judged iterations so far
    int64_t best_iter;     // 1-based iteration of the best total, 0: none yet
    int64_t since;         // judged iterations without an improvement since the best one
    int64_t stop_iter;     // 1-based iteration at which `stopped` was set, 0: not stopped
    double best;           // the best pooled total (+inf before the first one)
    int improved;          // verdict of the last judged iteration: the snapshot kernel copies when it is 1
    int stopped;           // patience ran out: best, best_iter and improved are frozen
    int bad;               // flag word of the list checks
    int pad_;
};

// bad[0] = 1 unless rows / cols are in range, rows non-decreasing and every value finite
template <typename T>
__global__ __launch_bounds__(256) void heldout_check_kernel(const int* __restrict__ rows, const int* __restrict__ cols, const T* __restrict__ vals,
                                                            int64_t n, int64_t n_i, int64_t n_j, int* __restrict__ bad) {
    int off = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int r = rows[e], c = cols[e];
        const T v = vals[e];
        if (r < 0 || (int64_t)r >= n_i || c < 0 || (int64_t)c >= n_j) off = 1;
        if (e > 0 && rows[e - 1] > r) off = 1;
        if (!(v - v == (T)0)) off = 1;                      // NaN and +-inf
    }
    if (off) *bad = 1;
}

// part[blockIdx.x] = the slab's sum of ((double)v - (double)x)^2 in the order of the header comment.  A workgroup is four
// waves; in pass p wave w holds the four entries 16 p + 4 w .. + 3 of the slab, 16 adjacent lanes each (the trip count is
// the workgroup's: the shuffles below).
template <typename T>
__global__ __launch_bounds__(HELDOUT_THREADS) void heldout_sqerr_kernel(const T* __restrict__ H, int64_t ldh, const T* __restrict__ Gc, int64_t ldg,
                                                                        int c, const int* __restrict__ rows, const int* __restrict__ cols,
                                                                        const T* __restrict__ vals, int64_t n, double* __restrict__ part) {
    __shared__ double res[HELDOUT_SLAB];
    const int t = threadIdx.x, lane = t & 63, g = lane & (ENTRY_LANES - 1), sub = lane / ENTRY_LANES, wave = t >> 6;
    const int64_t base = (int64_t)blockIdx.x * HELDOUT_SLAB;
    for (int pass = 0; pass < HELDOUT_SLAB / 16; ++pass) {
        const int slot = pass * 16 + wave * 4 + sub;
        const int64_t e = base + slot;
        T sum = 0;
        if (e < n) {
            const T* h = H + (int64_t)rows[e] * ldh;
            const T* gc = Gc + (int64_t)cols[e] * ldg;
            for (int q = g; q < c; q += ENTRY_LANES) sum += h[q] * gc[q];
        }
#pragma unroll
        for (int off = ENTRY_LANES / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, ENTRY_LANES);
        if (g == 0) {
#pragma clang fp contract(off)
            double sq = 0.0;
            if (e < n) {
                const double d = (double)vals[e] - (double)sum;
                sq = d * d;
            }
            res[slot] = sq;
        }
    }
    __syncthreads();
    const double a = ((res[t] + res[t + 256]) + res[t + 512]) + res[t + 768];
    __syncthreads();
    res[t] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) res[t] += res[t + w];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = res[0];
}

// One workgroup.  Thread l adds the partials of list l, off[l] .. off[l + 1], first to last, into cur[l]; thread 0 then
// judges (state != null): the history row of this iteration while capacity lasts, total = cur[0] + cur[1] + ... in list
// order, and the state words.  IMPROVEMENT: the first total that is not NaN (best is +inf until then), afterwards
// total < best - min_delta; a NaN total never improves.  Without one, `since` grows, and with patience > 0 and
// since >= patience the monitor stops: best, best_iter and improved stay as they are from then on.
static __global__ __launch_bounds__(256) void heldout_judge_kernel(const double* __restrict__ part, const int64_t* __restrict__ off, int n_lists,
                                                                   double* __restrict__ cur, HeldoutState* __restrict__ state,
                                                                   double* __restrict__ history, int64_t capacity, int patience, double min_delta) {
#pragma clang fp contract(off)
    for (int l = threadIdx.x; l < n_lists; l += blockDim.x) {
        double tot = 0.0;
        for (int64_t b = off[l]; b < off[l + 1]; ++b) tot += part[b];
        cur[l] = tot;
    }
    __syncthreads();
    if (threadIdx.x != 0 || !state) return;
    const int64_t it = state->seen;
    double total = 0.0;
    for (int l = 0; l < n_lists; ++l) {
        total += cur[l];
        if (it < capacity) history[it * n_lists + l] = cur[l];
    }
    state->seen = it + 1;
    if (state->stopped) return;
    const bool better = state->best_iter == 0 ? total == total : total < state->best - min_delta;
    if (better) {
        state->best = total;
        state->best_iter = it + 1;
        state->since = 0;
        state->improved = 1;
        return;
    }
    state->improved = 0;
    state->since += 1;
    if (patience > 0 && state->since >= (int64_t)patience) {
        state->stopped = 1;
        state->stop_iter = it + 1;
    }
}

// Every factor master and every backbone of the plan as word ranges; blockIdx.y names the range, the words by grid stride
// (16 bytes per lane, the tail in words).  All of it only when the last judged iteration improved.
struct HeldoutSeg {
    const unsigned* src;
    unsigned* dst;
    int64_t words;         // 4-byte words; src and dst are 256-byte aligned
};
struct alignas(16) HeldoutW4 { unsigned x, y, z, w; };

static __global__ __launch_bounds__(256) void heldout_snapshot_kernel(const HeldoutSeg* __restrict__ segs, const HeldoutState* __restrict__ state) {
    if (!state->improved) return;
    const HeldoutSeg s = segs[blockIdx.y];
    const int64_t quads = s.words >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    const HeldoutW4* s4 = (const HeldoutW4*)s.src;
    HeldoutW4* d4 = (HeldoutW4*)s.dst;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += stride) d4[i] = s4[i];
    for (int64_t i = 4 * quads + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < s.words; i += stride) s.dst[i] = s.src[i];
}

}  // namespace skf
