// skf_complete.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): the host side of the consuming operators skf_complete_topk / _entries / _ranks / _above / _digits /
// _hist / _row_kth (kernels: skf_complete.h), their C entry points included.  Every rule of the front end is stated once and named after what it checks;
// an entry point reads as its own order of them:
//   SKF_E_INVALID refusals (shape, operands, lists that come in pairs) -> SKF_E_WORKSPACE refusals -> the first HIP call
//   -> validation of the lists on the device -> the launches.
// A refused call writes no output.
static_assert(SKF_TOPK_MAX == SKF_TOPK_MAX_K, "include/skfusion_hip.h and skf_complete.h disagree on the list length");

// ---- the scored operands of a call, as the C ABI hands them over ------------------------------------------------------------
struct Scored {
    int32_t dtype;
    const void* H;  int64_t ldh, m;
    const void* Gc; int64_t ldg, n_cols;
    int32_t c;
    const int64_t* xptr; const int32_t* xidx;      // the exclusion lists (entries: none)
};

static size_t dtype_size(int32_t dtype) { return dtype == SKF_F64 ? 8 : 4; }

// f(T{}) with T = double or float: the ONE place a checked dtype becomes a template argument
template <class F>
static void by_dtype(int32_t dtype, F&& f) {
    if (dtype == SKF_F64) f(double{}); else f(float{});
}

// What a workspace query knows of the operands; `op` is the operator's name behind skf_complete_
static void check_shape(const char* op, int32_t dtype, int64_t m, int64_t n_cols) {
    if (dtype != SKF_F64 && dtype != SKF_F32) SKF_FAIL(SKF_E_INVALID, "skf_complete_%s: dtype must be SKF_F64 / SKF_F32", op);
    if (m < 0 || m >= (1LL << 31) || n_cols < 0 || n_cols >= (1LL << 31))
        SKF_FAIL(SKF_E_INVALID, "skf_complete_%s: m = %lld / n_cols = %lld outside 0 .. 2^31 - 1", op, (long long)m, (long long)n_cols);
}

// ... and what only the call knows (after check_shape: the two together are the operand check)
static void check_operands(const char* op, const Scored& s) {
    if (s.c < 1 || s.c > 1024) SKF_FAIL(SKF_E_INVALID, "skf_complete_%s: width c = %d outside 1 .. 1024", op, s.c);
    if (!s.H || !s.Gc) SKF_FAIL(SKF_E_INVALID, "skf_complete_%s: null argument", op);
    if (s.ldh < s.c || s.ldg < s.c) SKF_FAIL(SKF_E_INVALID, "skf_complete_%s: ld too small", op);
    if ((s.xptr == nullptr) != (s.xidx == nullptr))
        SKF_FAIL(SKF_E_INVALID, "skf_complete_%s: excl_indptr and excl_indices come together (both NULL: no exclusion)", op);
}

static void check_workspace(const char* op, const void* workspace, size_t have, size_t need) {
    if (!workspace || have < need)
        SKF_FAIL(SKF_E_WORKSPACE, "skf_complete_%s: workspace %zu B < required %zu B (or null)", op, workspace ? have : (size_t)0, need);
    if (((uintptr_t)workspace & 255) != 0) SKF_FAIL(SKF_E_WORKSPACE, "skf_complete_%s: workspace must be 256-byte aligned", op);
}

// The exclusion lists, on the device, before anything walks them: the number of entries is the list's own last pointer
// (one read-back), everything else is checked against it (one launch and its flag).  m > 0.
static void validate_exclusion(const char* op, const Scored& s, int* flag_word, hipStream_t st) {
    if (!s.xptr) return;
    int64_t nnz = -1;
    SKF_HIP(hipMemcpyAsync(&nnz, s.xptr + s.m, sizeof nnz, hipMemcpyDeviceToHost, st));
    SKF_HIP(hipStreamSynchronize(st));
    if (nnz < 0 || !csr_is_canonical(s.xptr, (const int*)s.xidx, s.m, s.n_cols, nnz, flag_word, st))
        SKF_FAIL(SKF_E_INVALID, "skf_complete_%s: the exclusion lists are not canonical for %lld rows x %lld columns (indptr from 0 "
                 "to the count, non-decreasing; indices in range and strictly ascending within a row)", op, (long long)s.m, (long long)s.n_cols);
}

// ---- the column splits ---------------------------------------------------------------------------------------------------------
// The ONE place the column splits of a pass over the score tiles are decided: the workspace query and the launch both call
// it, so a query with col_splits = 0 sizes for what the launch will choose.  A split is a whole number of 64-column tiles; a
// chosen count aims at two workgroups per compute unit (256 CUs) and keeps at least four tiles per split, so that the partial
// lists and their merge stay small next to the pass; a requested count is only clamped to what exists.
static int topk_col_splits(int64_t m, int64_t n_cols, int want) {
    const int64_t ntiles = std::max<int64_t>(1, (n_cols + TOPK_BN - 1) / TOPK_BN);
    const int64_t row_tiles = std::max<int64_t>(1, (m + TOPK_BM - 1) / TOPK_BM);
    int64_t s = want;
    if (want <= 0) {
        s = (512 + row_tiles - 1) / row_tiles;
        s = std::min<int64_t>(s, std::max<int64_t>(1, ntiles / 4));
    }
    s = std::min<int64_t>(std::min<int64_t>(s, TOPK_MAX_SPLITS), ntiles);
    return (int)std::max<int64_t>(1, s);
}

// A requested col_splits above TOPK_MAX_SPLITS.  The contract of skf_complete_topk (include/skfusion_hip.h) promises a cut
// into "at most 32 parts and never more than there are tiles": any count is a wish that topk_col_splits clamps, and its
// callers may rely on that.  The contracts of ranks and above give col_splits a range, 0 .. 32, and a value outside a
// documented range is refused like any other.  Both rules are part of the ABI; neither is an oversight.
enum OverMaxSplits { OVER_MAX_CLAMP, OVER_MAX_REFUSE };
static void check_col_splits(const char* op, int32_t col_splits, OverMaxSplits over_max) {
    if (over_max == OVER_MAX_CLAMP) {
        if (col_splits < 0) SKF_FAIL(SKF_E_INVALID, "skf_complete_%s: col_splits = %d is negative", op, col_splits);
    } else if (col_splits < 0 || col_splits > TOPK_MAX_SPLITS) {
        SKF_FAIL(SKF_E_INVALID, "skf_complete_%s: col_splits = %d outside 0 .. %d", op, col_splits, TOPK_MAX_SPLITS);
    }
}

// the operands every pass's argument block begins with (TopkArgs / RankArgs / AboveArgs / DigitArgs / HistArgs / RowDigitArgs<T>, skf_complete.h),
// tiles_per_split included
template <typename T, template <typename> class Args>
static void fill_operands(Args<T>& a, const Scored& s, int splits) {
    a.H = (const T*)s.H; a.ldh = s.ldh; a.m = s.m;
    a.Gc = (const T*)s.Gc; a.ldg = s.ldg; a.n_cols = s.n_cols;
    a.c = s.c;
    a.xptr = s.xptr; a.xidx = (const int*)s.xidx;
    const int64_t ntiles = (s.n_cols + TOPK_BN - 1) / TOPK_BN;
    a.tiles_per_split = (int)std::max<int64_t>(1, (ntiles + splits - 1) / splits);
}

// ---- top-k ---------------------------------------------------------------------------------------------------------------------
// [0, 256): the flag of the exclusion check; then, for more than one split, the partial lists: values [splits][m][k],
// indices [splits][m][k]
static size_t topk_workspace(size_t esz, int64_t m, int k, int splits) {
    size_t b = 256;
    if (splits > 1) b += align_up((size_t)splits * m * k * esz, 256) + align_up((size_t)splits * m * k * sizeof(int), 256);
    return b;
}

static void topk_check_query(int32_t dtype, int64_t m, int64_t n_cols, int32_t k, int32_t col_splits) {
    check_shape("topk", dtype, m, n_cols);
    if (k < 1 || k > SKF_TOPK_MAX) SKF_FAIL(SKF_E_INVALID, "skf_complete_topk: k = %d outside 1 .. %d", k, SKF_TOPK_MAX);
    check_col_splits("topk", col_splits, OVER_MAX_CLAMP);
}

template <typename T>
static void launch_complete_topk(const Scored& s, int k, int* out_idx, int64_t ld_idx, void* out_val, int64_t ld_val, int splits,
                                 char* ws, hipStream_t st) {
    TopkArgs<T> a;
    fill_operands(a, s, splits);
    a.k = k;
    a.out_idx = out_idx; a.ld_idx = ld_idx; a.out_val = (T*)out_val; a.ld_val = ld_val;
    a.part_val = (T*)(ws + 256);
    a.part_idx = (int*)(ws + 256 + align_up((size_t)splits * s.m * k * sizeof(T), 256));
    static DeviceOnce once;
    allow_dynamic_lds(once, complete_topk_kernel<T>, (int)topk_list_bytes(SKF_TOPK_MAX, sizeof(T)));
    hipLaunchKernelGGL((complete_topk_kernel<T>), dim3(cdiv(s.m, TOPK_BM), splits), dim3(TOPK_THREADS), topk_list_bytes(k, sizeof(T)), st, a);
    check_launch("complete_topk");
    if (splits > 1) {
        hipLaunchKernelGGL((complete_topk_merge_kernel<T>), dim3(elem_grid(s.m)), dim3(256), 0, st, a.part_idx, a.part_val, s.m, k, splits,
                           out_idx, ld_idx, (T*)out_val, ld_val);
        check_launch("complete_topk_merge");
    }
}

// ---- entries -------------------------------------------------------------------------------------------------------------------
template <typename T>
static void launch_complete_entries(const Scored& s, const int* rows, const int* cols, int64_t n, void* out, hipStream_t st) {
    const int64_t waves = (n + 3) / 4;                      // four entries per wave and step
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, 4096));
    hipLaunchKernelGGL((complete_entries_kernel<T>), dim3(grid), dim3(256), 0, st, (const T*)s.H, s.ldh, (const T*)s.Gc, s.ldg, s.c, rows,
                       cols, n, (T*)out);
    check_launch("complete_entries");
}

// ---- ranks of given pairs --------------------------------------------------------------------------------------------------------
// Workspace: [0, 256) the flag word of the list checks; [256, 512) the RANK_MAX_PARTS partial maxima of
// rank_longest_row_kernel; then the scores of the targets, used when the caller keeps none (out_val NULL) -- the query
// cannot know and sizes for them.  Nothing here grows with m x n_cols.
static size_t ranks_workspace(size_t esz, int64_t n_targets) { return 512 + align_up((size_t)n_targets * esz, 256); }

static void ranks_check_query(int32_t dtype, int64_t m, int64_t n_cols, int64_t n_targets, int32_t col_splits) {
    check_shape("ranks", dtype, m, n_cols);
    if (n_targets < 0) SKF_FAIL(SKF_E_INVALID, "skf_complete_ranks: n_targets = %lld is negative", (long long)n_targets);
    check_col_splits("ranks", col_splits, OVER_MAX_REFUSE);
}

template <typename T>
static void launch_complete_ranks(const Scored& s, const int64_t* tptr, const int* tidx, int* out_rank, void* val, int splits,
                                  int64_t longest, hipStream_t st) {
    RankArgs<T> a;
    fill_operands(a, s, splits);
    a.tptr = tptr; a.tidx = tidx;
    a.out_rank = out_rank; a.val = (T*)val;
    const int row_tiles = cdiv(s.m, TOPK_BM);
    hipLaunchKernelGGL((complete_rank_scores_kernel<T>), dim3(row_tiles), dim3(TOPK_THREADS), 0, st, a);
    check_launch("complete_rank_scores");
    // one workgroup per chunk of the longest row (a workgroup strides over the chunks beyond what one grid dimension holds)
    const int64_t chunks = (longest + RANK_CHUNK - 1) / RANK_CHUNK;
    a.chunk_groups = (int)std::max<int64_t>(1, std::min<int64_t>(chunks, 0x7fffffff / row_tiles));
    static DeviceOnce once;
    allow_dynamic_lds(once, complete_rank_count_kernel<T>, (int)rank_chunk_bytes(sizeof(T)));
    hipLaunchKernelGGL((complete_rank_count_kernel<T>), dim3((unsigned)a.chunk_groups * row_tiles, splits), dim3(TOPK_THREADS), rank_chunk_bytes(sizeof(T)), st, a);
    check_launch("complete_rank_count");
}

// ---- every pair at or above a threshold ----------------------------------------------------------------------------------------
// Workspace: [0, 256) the flag word of the exclusion check; then the ABOVE_SCAN_PARTS chunk sums of the scan; then one int64
// per (split, row): the counts of the count pass, turned into the starts of the fill pass in place.  Nothing here grows with
// m x n_cols.
static size_t above_workspace(int64_t m, int splits) {
    return 256 + ABOVE_SCAN_PARTS * sizeof(int64_t) + align_up((size_t)splits * (size_t)m * sizeof(int64_t), 256);
}

static void above_check_query(int32_t dtype, int64_t m, int64_t n_cols, int32_t col_splits) {
    check_shape("above", dtype, m, n_cols);
    check_col_splits("above", col_splits, OVER_MAX_REFUSE);
}

// the count pass and the scan: out_indptr (the total at [m]) and the (row, split) starts in the workspace
template <typename T>
static void launch_above_count(const AboveArgs<T>& a, int splits, char* ws, int64_t* out_indptr, hipStream_t st) {
    const int row_tiles = cdiv(a.m, TOPK_BM);
    hipLaunchKernelGGL((complete_above_kernel<T, false>), dim3(row_tiles, splits), dim3(TOPK_THREADS), 0, st, a);
    check_launch("complete_above_count");
    int64_t* parts = (int64_t*)(ws + 256);
    const int64_t want = std::min<int64_t>(ABOVE_SCAN_PARTS, (a.m + 255) / 256);
    const int64_t chunk = ((a.m + want - 1) / want + 255) / 256 * 256;           // rows per workgroup: a multiple of 256
    const int nparts = (int)((a.m + chunk - 1) / chunk);
    hipLaunchKernelGGL(above_chunk_sums_kernel, dim3(nparts), dim3(256), 0, st, (const int64_t*)a.work, a.m, splits, chunk, parts);
    check_launch("above_chunk_sums");
    hipLaunchKernelGGL(above_chunk_starts_kernel, dim3(1), dim3(256), 0, st, parts, nparts, a.m, out_indptr);
    check_launch("above_chunk_starts");
    hipLaunchKernelGGL(above_offsets_kernel, dim3(nparts), dim3(256), 0, st, a.work, a.m, splits, chunk, (const int64_t*)parts, out_indptr);
    check_launch("above_offsets");
}

// count, scan, ONE read-back of the total, then -- unless the caller asked for the count alone or has too little room -- fill
template <typename T>
static void run_complete_above(const Scored& s, const void* thr, int64_t capacity, int64_t* out_indptr, int* out_indices, void* out_values,
                               int64_t* n_found, int splits, char* ws, hipStream_t st) {
    AboveArgs<T> a;
    fill_operands(a, s, splits);
    a.thr = (const T*)thr;
    a.work = (int64_t*)(ws + 256 + ABOVE_SCAN_PARTS * sizeof(int64_t));
    a.indptr = out_indptr;
    a.out_indices = out_indices; a.out_values = (T*)out_values;
    launch_above_count<T>(a, splits, ws, out_indptr, st);
    int64_t total = -1;
    SKF_HIP(hipMemcpyAsync(&total, out_indptr + s.m, sizeof total, hipMemcpyDeviceToHost, st));
    SKF_HIP(hipStreamSynchronize(st));
    *n_found = total;
    if (!out_indices) return;                           // count only
    if (total > capacity)
        SKF_FAIL(SKF_E_WORKSPACE, "skf_complete_above: %lld entries found, capacity %lld (out_indptr and *n_found are written: "
                 "call again with that capacity)", (long long)total, (long long)capacity);
    if (total > 0) {
        hipLaunchKernelGGL((complete_above_kernel<T, true>), dim3(cdiv(s.m, TOPK_BM), splits), dim3(TOPK_THREADS), 0, st, a);
        check_launch("complete_above_fill");
    }
}

// ---- one digit of the radix select over every candidate score -----------------------------------------------------------------
// Workspace: [0, 256) the flag word of the exclusion check, nothing else: the histogram is the caller's.
static size_t digits_workspace() { return 256; }

static void digits_check_query(int32_t dtype, int64_t m, int64_t n_cols, int32_t col_splits) {
    check_shape("digits", dtype, m, n_cols);
    check_col_splits("digits", col_splits, OVER_MAX_REFUSE);
}

// the digit asked for lies inside the key of the scoring type, and the prefix inside its own bits
static void check_digit(int32_t dtype, uint64_t prefix, int32_t prefix_bits, int32_t digit_bits) {
    const int key_bits = 8 * (int)dtype_size(dtype);
    if (digit_bits < 1 || digit_bits > DIGIT_MAX_BITS)
        SKF_FAIL(SKF_E_INVALID, "skf_complete_digits: digit_bits = %d outside 1 .. %d", digit_bits, DIGIT_MAX_BITS);
    if (prefix_bits < 0 || prefix_bits > key_bits - digit_bits)
        SKF_FAIL(SKF_E_INVALID, "skf_complete_digits: prefix_bits = %d with digit_bits = %d outside the %d key bits", prefix_bits,
                 digit_bits, key_bits);
    if ((prefix >> prefix_bits) != 0)                   // (prefix_bits <= 63 here)
        SKF_FAIL(SKF_E_INVALID, "skf_complete_digits: prefix %llu does not fit its %d bits", (unsigned long long)prefix, prefix_bits);
}

template <typename T>
static void launch_complete_digits(const Scored& s, uint64_t prefix, int prefix_bits, int digit_bits, uint64_t* hist, int splits,
                                   hipStream_t st) {
    DigitArgs<T> a;
    fill_operands(a, s, splits);
    a.prefix = prefix; a.prefix_bits = prefix_bits; a.digit_bits = digit_bits;
    a.hist = (unsigned long long*)hist;
    hipLaunchKernelGGL((complete_digits_kernel<T>), dim3(cdiv(s.m, TOPK_BM), splits), dim3(TOPK_THREADS), 0, st, a);
    check_launch("complete_digits");
}

// ---- the histogram of every candidate score by value, and of given pairs -----------------------------------------------------
// Workspace: [0, 256) three verdict words -- the exclusion lists, the target lists, the edges --, nothing else: the histograms
// are the caller's.
static_assert(SKF_HIST_MAX_EDGES == HIST_MAX_EDGES, "include/skfusion_hip.h and skf_complete.h disagree on the number of edges");
static size_t hist_workspace() { return 256; }

static void hist_check_query(int32_t dtype, int64_t m, int64_t n_cols, int64_t n_targets, int32_t col_splits) {
    check_shape("hist", dtype, m, n_cols);
    if (n_targets < 0) SKF_FAIL(SKF_E_INVALID, "skf_complete_hist: n_targets = %lld is negative", (long long)n_targets);
    check_col_splits("hist", col_splits, OVER_MAX_REFUSE);
}

// The exclusion lists, the target lists (tptr[m] == n_targets is part of their check) and the edges, each by its own kernel
// into its own verdict word, read back together: one round trip (and, as for every operator, the read-back of the exclusion
// lists' own count ahead of it).  m > 0.
template <typename T>
static void validate_hist(const Scored& s, const int64_t* tptr, const int* tidx, int64_t n_targets, const void* edges, int n_edges,
                          int* flags, hipStream_t st) {
    int64_t nnz = 0;
    if (s.xptr) {
        SKF_HIP(hipMemcpyAsync(&nnz, s.xptr + s.m, sizeof nnz, hipMemcpyDeviceToHost, st));
        SKF_HIP(hipStreamSynchronize(st));
    }
    int bad[3] = {nnz < 0, 0, 0};
    if (!bad[0]) {
        SKF_HIP(hipMemsetAsync(flags, 0, sizeof bad, st));
        if (s.xptr) {
            hipLaunchKernelGGL(known_csr_check_kernel, dim3(wave_grid(s.m)), dim3(256), 0, st, s.xptr, (const int*)s.xidx, s.m, s.n_cols, nnz, flags);
            check_launch("known_csr_check");
        }
        if (tptr) {
            hipLaunchKernelGGL(known_csr_check_kernel, dim3(wave_grid(s.m)), dim3(256), 0, st, tptr, tidx, s.m, s.n_cols, n_targets, flags + 1);
            check_launch("known_csr_check");
        }
        hipLaunchKernelGGL((hist_edges_check_kernel<T>), dim3(cdiv(n_edges, 256)), dim3(256), 0, st, (const T*)edges, n_edges, flags + 2);
        check_launch("hist_edges_check");
        SKF_HIP(hipMemcpyAsync(bad, flags, sizeof bad, hipMemcpyDeviceToHost, st));
        SKF_HIP(hipStreamSynchronize(st));
    }
    if (bad[0])
        SKF_FAIL(SKF_E_INVALID, "skf_complete_hist: the exclusion lists are not canonical for %lld rows x %lld columns (indptr from 0 "
                 "to the count, non-decreasing; indices in range and strictly ascending within a row)", (long long)s.m, (long long)s.n_cols);
    if (bad[1])
        SKF_FAIL(SKF_E_INVALID, "skf_complete_hist: the target lists are not canonical for %lld rows x %lld columns and %lld targets "
                 "(indptr from 0 to the count, non-decreasing; indices in range and strictly ascending within a row)",
                 (long long)s.m, (long long)s.n_cols, (long long)n_targets);
    if (bad[2]) SKF_FAIL(SKF_E_INVALID, "skf_complete_hist: the %d edges hold a NaN or descend", n_edges);
}

template <typename T>
static void launch_complete_hist(const Scored& s, const int64_t* tptr, const int* tidx, const void* edges, int n_edges, uint64_t* hist,
                                 uint64_t* hist_tgt, int splits, hipStream_t st) {
    HistArgs<T> a;
    fill_operands(a, s, splits);
    a.tptr = tptr; a.tidx = tidx;
    a.edges = (const T*)edges; a.n_edges = n_edges; a.steps = hist_steps(n_edges);
    a.hist = (unsigned long long*)hist; a.hist_tgt = (unsigned long long*)hist_tgt;
    static DeviceOnce once;
    allow_dynamic_lds(once, complete_hist_kernel<T>, (int)hist_lds_bytes(HIST_MAX_EDGES, true, sizeof(T)));
    hipLaunchKernelGGL((complete_hist_kernel<T>), dim3(cdiv(s.m, TOPK_BM), splits), dim3(TOPK_THREADS),
                       hist_lds_bytes(n_edges, tptr != nullptr, sizeof(T)), st, a);
    check_launch("complete_hist");
}

// ---- the k-th best score of every row ------------------------------------------------------------------------------------------
// Workspace: [0, 256) the flag word of the checks; the row histograms, uint32 [m][ROW_BINS]; one key prefix and one `need`
// word per row.  It grows with m, never with m x n_cols.
static size_t row_kth_workspace(int64_t m) {
    return 256 + align_up((size_t)m * ROW_BINS * sizeof(unsigned), 256) + 2 * align_up((size_t)m * sizeof(int64_t), 256);
}

static void row_kth_check_query(int32_t dtype, int64_t m, int64_t n_cols, int32_t col_splits) {
    check_shape("row_kth", dtype, m, n_cols);
    check_col_splits("row_kth", col_splits, OVER_MAX_REFUSE);
}

// validate_exclusion and, under the same verdict word and read-back, want[r] >= 0.  m > 0.
static void validate_row_kth(const Scored& s, const int64_t* want, int* flag_word, hipStream_t st) {
    int64_t nnz = 0;
    if (s.xptr) {
        SKF_HIP(hipMemcpyAsync(&nnz, s.xptr + s.m, sizeof nnz, hipMemcpyDeviceToHost, st));
        SKF_HIP(hipStreamSynchronize(st));
    }
    const int bad = nnz < 0 ? 1 : device_flag(flag_word, st, [&] {
        if (s.xptr) {
            hipLaunchKernelGGL(known_csr_check_kernel, dim3(wave_grid(s.m)), dim3(256), 0, st, s.xptr, (const int*)s.xidx, s.m, s.n_cols, nnz, flag_word);
            check_launch("known_csr_check");
        }
        hipLaunchKernelGGL(row_want_check_kernel, dim3(elem_grid(s.m)), dim3(256), 0, st, want, s.m, flag_word);
        check_launch("row_want_check");
    });
    if (bad == 1)
        SKF_FAIL(SKF_E_INVALID, "skf_complete_row_kth: the exclusion lists are not canonical for %lld rows x %lld columns (indptr from 0 "
                 "to the count, non-decreasing; indices in range and strictly ascending within a row)", (long long)s.m, (long long)s.n_cols);
    if (bad) SKF_FAIL(SKF_E_INVALID, "skf_complete_row_kth: a want[r] is negative");
}

// every pass and every walk of the select, enqueued: no host round trip in between
template <typename T>
static void launch_complete_row_kth(const Scored& s, const int64_t* want, void* thr, int64_t* greater, int64_t* equal, int64_t* cands,
                                    int splits, char* ws, hipStream_t st) {
    constexpr int KEY_BITS = ScoreKey<T>::BITS;
    RowDigitArgs<T> a;
    fill_operands(a, s, splits);
    a.hist = (unsigned*)(ws + 256);
    unsigned long long* prefix = (unsigned long long*)(ws + 256 + align_up((size_t)s.m * ROW_BINS * sizeof(unsigned), 256));
    int64_t* need = (int64_t*)((char*)prefix + align_up((size_t)s.m * sizeof(int64_t), 256));
    a.prefix = prefix; a.need = need;
    RowWalkArgs w = {a.hist, s.m, 0, 0, 0, want, prefix, need, greater, equal, cands, thr};
    SKF_HIP(hipMemsetAsync(a.hist, 0, (size_t)s.m * ROW_BINS * sizeof(unsigned), st));
    static DeviceOnce once;
    allow_dynamic_lds(once, complete_row_digits_kernel<T>, (int)row_bins_bytes());
    // no column: no candidate -- one walk over the empty histograms writes NaN / 0 to every row
    for (int pbits = 0; pbits < KEY_BITS;) {
        const int db = s.n_cols == 0 ? KEY_BITS : std::min(ROW_DIGIT_BITS, KEY_BITS - pbits);
        if (s.n_cols > 0) {
            a.prefix_bits = pbits; a.digit_bits = db;
            hipLaunchKernelGGL((complete_row_digits_kernel<T>), dim3(cdiv(s.m, TOPK_BM), splits), dim3(TOPK_THREADS), row_bins_bytes(), st, a);
            check_launch("complete_row_digits");
        }
        w.digit_bits = db; w.first = pbits == 0; w.last = pbits + db == KEY_BITS;
        hipLaunchKernelGGL((complete_row_walk_kernel<T>), dim3(wave_grid(s.m)), dim3(256), 0, st, w);
        check_launch("complete_row_walk");
        pbits += db;
    }
}

// ---- the C entry points --------------------------------------------------------------------------------------------------------
// When there is nothing to score the three list operators differ, on purpose: top-k leaves at m == 0 (no row to write; with
// n_cols == 0 it still validates and launches: every slot gets -1 / -inf), ranks leaves at n_targets == 0 before any list
// is read, and above validates its exclusion lists whenever there is a row, n_cols == 0 included: it is the one operator that
// still writes outputs then (out_indptr all zero, *n_found = 0), and "every refusal leaves every output as it was" holds there too.
extern "C" {

int skf_complete_topk_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int32_t k, int32_t col_splits, size_t* bytes) {
    return guarded([&] {
        if (!bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        topk_check_query(dtype, m, n_cols, k, col_splits);
        *bytes = topk_workspace(dtype_size(dtype), m, k, topk_col_splits(m, n_cols, col_splits));
    });
}

int skf_complete_topk(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols, int32_t c,
                      int32_t k, const int64_t* excl_indptr, const int32_t* excl_indices, int32_t* out_idx, int64_t ld_idx,
                      void* out_val, int64_t ld_val, int32_t col_splits, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] {
        const Scored s = {dtype, H, ldh, m, Gc, ldg, n_cols, c, excl_indptr, excl_indices};
        topk_check_query(dtype, m, n_cols, k, col_splits);
        check_operands("topk", s);
        if (!out_idx || !out_val) SKF_FAIL(SKF_E_INVALID, "skf_complete_topk: null argument");
        if (ld_idx < k || ld_val < k) SKF_FAIL(SKF_E_INVALID, "skf_complete_topk: ld too small");
        const int splits = topk_col_splits(m, n_cols, col_splits);
        check_workspace("topk", workspace, workspace_bytes, topk_workspace(dtype_size(dtype), m, k, splits));
        if (m == 0) return;
        hipStream_t st = as_stream(stream);
        validate_exclusion("topk", s, (int*)workspace, st);
        by_dtype(dtype, [&](auto t) {
            launch_complete_topk<decltype(t)>(s, k, out_idx, ld_idx, out_val, ld_val, splits, (char*)workspace, st);
        });
    });
}

int skf_complete_entries(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols, int32_t c,
                         const int32_t* rows, const int32_t* cols, int64_t n, void* out, void* stream) {
    return guarded([&] {
        const Scored s = {dtype, H, ldh, m, Gc, ldg, n_cols, c, nullptr, nullptr};
        check_shape("entries", dtype, m, n_cols);
        if (n < 0) SKF_FAIL(SKF_E_INVALID, "skf_complete_entries: n = %lld is negative", (long long)n);
        check_operands("entries", s);
        if (!rows || !cols || !out) SKF_FAIL(SKF_E_INVALID, "skf_complete_entries: null argument");
        if (n == 0) return;
        hipStream_t st = as_stream(stream);
        // the index check needs one device word and this operator has no workspace: the first word of `out` serves (every
        // out[e] is overwritten by the pass) and gets its old content back when the entries are refused
        int keep = 0;
        int* flag = (int*)out;
        SKF_HIP(hipMemcpyAsync(&keep, flag, sizeof(int), hipMemcpyDeviceToHost, st));
        const int bad = device_flag(flag, st, [&] {
            hipLaunchKernelGGL(complete_entries_check_kernel, dim3(elem_grid(n)), dim3(256), 0, st, (const int*)rows, (const int*)cols, n, m, n_cols, flag);
            check_launch("complete_entries_check");
        });
        if (bad) {
            SKF_HIP(hipMemcpyAsync(flag, &keep, sizeof(int), hipMemcpyHostToDevice, st));
            SKF_HIP(hipStreamSynchronize(st));
            SKF_FAIL(SKF_E_INVALID, "skf_complete_entries: an entry names a row outside 0 .. %lld or a column outside 0 .. %lld",
                     (long long)m - 1, (long long)n_cols - 1);
        }
        by_dtype(dtype, [&](auto t) { launch_complete_entries<decltype(t)>(s, (const int*)rows, (const int*)cols, n, out, st); });
    });
}

int skf_complete_ranks_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int64_t n_targets, int32_t col_splits, size_t* bytes) {
    return guarded([&] {
        if (!bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        ranks_check_query(dtype, m, n_cols, n_targets, col_splits);
        *bytes = ranks_workspace(dtype_size(dtype), n_targets);
    });
}

int skf_complete_ranks(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols, int32_t c,
                       const int64_t* tgt_indptr, const int32_t* tgt_indices, int64_t n_targets, const int64_t* excl_indptr,
                       const int32_t* excl_indices, int32_t* out_rank, void* out_val, int32_t col_splits, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return guarded([&] {
        const Scored s = {dtype, H, ldh, m, Gc, ldg, n_cols, c, excl_indptr, excl_indices};
        ranks_check_query(dtype, m, n_cols, n_targets, col_splits);
        check_operands("ranks", s);
        if (!out_rank || !tgt_indptr || !tgt_indices) SKF_FAIL(SKF_E_INVALID, "skf_complete_ranks: null argument");
        check_workspace("ranks", workspace, workspace_bytes, ranks_workspace(dtype_size(dtype), n_targets));
        if (n_targets == 0) return;
        hipStream_t st = as_stream(stream);
        char* ws = (char*)workspace;
        // the target lists against the caller's count (tgt_indptr[m] == n_targets is part of the check), and in the same
        // round trip the longest row, which sizes the chunk grid (read only once the lists have passed)
        int* parts = (int*)(ws + 256);
        const int nparts = (int)std::max<int64_t>(1, std::min<int64_t>(RANK_MAX_PARTS, (m + 255) / 256));
        SKF_HIP(hipMemsetAsync(parts, 0, RANK_MAX_PARTS * sizeof(int), st));
        if (!csr_is_canonical(tgt_indptr, (const int*)tgt_indices, m, n_cols, n_targets, (int*)ws, st, [&] {
                hipLaunchKernelGGL(rank_longest_row_kernel, dim3(nparts), dim3(256), 0, st, tgt_indptr, m, parts);
                check_launch("rank_longest_row");
            }))
            SKF_FAIL(SKF_E_INVALID, "skf_complete_ranks: the target lists are not canonical for %lld rows x %lld columns and %lld targets "
                     "(indptr from 0 to the count, non-decreasing; indices in range and strictly ascending within a row)",
                     (long long)m, (long long)n_cols, (long long)n_targets);
        validate_exclusion("ranks", s, (int*)ws, st);
        int longest[RANK_MAX_PARTS];
        SKF_HIP(hipMemcpyAsync(longest, parts, sizeof longest, hipMemcpyDeviceToHost, st));
        SKF_HIP(hipStreamSynchronize(st));
        const int64_t longest_row = *std::max_element(longest, longest + RANK_MAX_PARTS);
        const int splits = topk_col_splits(m, n_cols, col_splits);
        void* val = out_val ? out_val : (void*)(ws + 512);
        by_dtype(dtype, [&](auto t) {
            launch_complete_ranks<decltype(t)>(s, tgt_indptr, (const int*)tgt_indices, out_rank, val, splits, longest_row, st);
        });
    });
}

int skf_complete_above_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int32_t col_splits, size_t* bytes) {
    return guarded([&] {
        if (!bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        above_check_query(dtype, m, n_cols, col_splits);
        *bytes = above_workspace(m, topk_col_splits(m, n_cols, col_splits));
    });
}

int skf_complete_above(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols, int32_t c,
                       const void* thr, const int64_t* excl_indptr, const int32_t* excl_indices, int64_t capacity, int64_t* out_indptr,
                       int32_t* out_indices, void* out_values, int64_t* n_found, int32_t col_splits, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return guarded([&] {
        const Scored s = {dtype, H, ldh, m, Gc, ldg, n_cols, c, excl_indptr, excl_indices};
        above_check_query(dtype, m, n_cols, col_splits);
        check_operands("above", s);
        if (!thr || !out_indptr || !n_found) SKF_FAIL(SKF_E_INVALID, "skf_complete_above: null argument");
        if (out_values && !out_indices) SKF_FAIL(SKF_E_INVALID, "skf_complete_above: out_values without out_indices");
        if (capacity < 0) SKF_FAIL(SKF_E_INVALID, "skf_complete_above: capacity = %lld is negative", (long long)capacity);
        const int splits = topk_col_splits(m, n_cols, col_splits);
        check_workspace("above", workspace, workspace_bytes, above_workspace(m, splits));
        hipStream_t st = as_stream(stream);
        if (m > 0) validate_exclusion("above", s, (int*)workspace, st);
        if (m == 0 || n_cols == 0) {                    // nothing to score: every row is empty
            SKF_HIP(hipMemsetAsync(out_indptr, 0, (size_t)(m + 1) * sizeof(int64_t), st));
            SKF_HIP(hipStreamSynchronize(st));
            *n_found = 0;
            return;
        }
        by_dtype(dtype, [&](auto t) {
            run_complete_above<decltype(t)>(s, thr, capacity, out_indptr, out_indices, out_values, n_found, splits, (char*)workspace, st);
        });
    });
}

int skf_complete_digits_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int32_t col_splits, size_t* bytes) {
    return guarded([&] {
        if (!bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        digits_check_query(dtype, m, n_cols, col_splits);
        *bytes = digits_workspace();
    });
}

int skf_complete_digits(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols, int32_t c,
                        const int64_t* excl_indptr, const int32_t* excl_indices, uint64_t prefix, int32_t prefix_bits,
                        int32_t digit_bits, uint64_t* hist, int32_t col_splits, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] {
        const Scored s = {dtype, H, ldh, m, Gc, ldg, n_cols, c, excl_indptr, excl_indices};
        digits_check_query(dtype, m, n_cols, col_splits);
        check_operands("digits", s);
        check_digit(dtype, prefix, prefix_bits, digit_bits);
        if (!hist) SKF_FAIL(SKF_E_INVALID, "skf_complete_digits: null argument");
        const int splits = topk_col_splits(m, n_cols, col_splits);
        check_workspace("digits", workspace, workspace_bytes, digits_workspace());
        if (m == 0) return;
        hipStream_t st = as_stream(stream);
        validate_exclusion("digits", s, (int*)workspace, st);
        if (n_cols == 0) return;                        // no column: no candidate
        by_dtype(dtype, [&](auto t) {
            launch_complete_digits<decltype(t)>(s, prefix, prefix_bits, digit_bits, hist, splits, st);
        });
    });
}

int skf_complete_hist_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int64_t n_targets, int32_t col_splits, size_t* bytes) {
    return guarded([&] {
        if (!bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        hist_check_query(dtype, m, n_cols, n_targets, col_splits);
        *bytes = hist_workspace();
    });
}

int skf_complete_hist(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols, int32_t c,
                      const void* edges, int32_t n_edges, const int64_t* excl_indptr, const int32_t* excl_indices,
                      const int64_t* tgt_indptr, const int32_t* tgt_indices, int64_t n_targets, uint64_t* hist, uint64_t* hist_tgt,
                      int32_t col_splits, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] {
        const Scored s = {dtype, H, ldh, m, Gc, ldg, n_cols, c, excl_indptr, excl_indices};
        hist_check_query(dtype, m, n_cols, n_targets, col_splits);
        check_operands("hist", s);
        if (n_edges < 1 || n_edges > SKF_HIST_MAX_EDGES)
            SKF_FAIL(SKF_E_INVALID, "skf_complete_hist: n_edges = %d outside 1 .. %d", n_edges, SKF_HIST_MAX_EDGES);
        if (!edges || !hist) SKF_FAIL(SKF_E_INVALID, "skf_complete_hist: null argument");
        if ((tgt_indptr == nullptr) != (tgt_indices == nullptr) || (tgt_indptr == nullptr) != (hist_tgt == nullptr))
            SKF_FAIL(SKF_E_INVALID, "skf_complete_hist: tgt_indptr, tgt_indices and hist_tgt come together (all NULL: no targets)");
        if (!tgt_indptr && n_targets != 0) SKF_FAIL(SKF_E_INVALID, "skf_complete_hist: n_targets = %lld without target lists", (long long)n_targets);
        const int splits = topk_col_splits(m, n_cols, col_splits);
        check_workspace("hist", workspace, workspace_bytes, hist_workspace());
        if (m == 0) return;
        hipStream_t st = as_stream(stream);
        by_dtype(dtype, [&](auto t) {
            validate_hist<decltype(t)>(s, tgt_indptr, (const int*)tgt_indices, n_targets, edges, n_edges, (int*)workspace, st);
        });
        if (n_cols == 0) return;                        // no column: no candidate
        by_dtype(dtype, [&](auto t) {
            launch_complete_hist<decltype(t)>(s, tgt_indptr, (const int*)tgt_indices, edges, n_edges, hist, hist_tgt, splits, st);
        });
    });
}

int skf_complete_row_kth_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int32_t col_splits, size_t* bytes) {
    return guarded([&] {
        if (!bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        row_kth_check_query(dtype, m, n_cols, col_splits);
        *bytes = row_kth_workspace(m);
    });
}

int skf_complete_row_kth(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols, int32_t c,
                         const int64_t* want, const int64_t* excl_indptr, const int32_t* excl_indices, void* out_thr,
                         int64_t* out_greater, int64_t* out_equal, int64_t* out_cands, int32_t col_splits, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return guarded([&] {
        const Scored s = {dtype, H, ldh, m, Gc, ldg, n_cols, c, excl_indptr, excl_indices};
        row_kth_check_query(dtype, m, n_cols, col_splits);
        check_operands("row_kth", s);
        if (!want || !out_thr || !out_greater || !out_equal) SKF_FAIL(SKF_E_INVALID, "skf_complete_row_kth: null argument");
        const int splits = topk_col_splits(m, n_cols, col_splits);
        check_workspace("row_kth", workspace, workspace_bytes, row_kth_workspace(m));
        if (m == 0) return;
        hipStream_t st = as_stream(stream);
        validate_row_kth(s, want, (int*)workspace, st);
        by_dtype(dtype, [&](auto t) {
            launch_complete_row_kth<decltype(t)>(s, want, out_thr, out_greater, out_equal, out_cands, splits, (char*)workspace, st);
        });
    });
}

}  // extern "C"
