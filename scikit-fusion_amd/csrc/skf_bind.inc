// skf_bind.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): everything that runs ONCE per plan when its workspace is bound (skf_plan_bind_workspace) -- the
// lists of every relation kept as its entries, the mask and bf16 copies, the constraint CSR, the tables of the
// pseudo-inverse and of the small-graph schedule -- and nothing that runs per iteration.  Bind is not on the hot path:
// the steps synchronise wherever a host vector has to outlive a copy.
// ------------------------------------------------------------------------------------------

// A device word as a verdict: cleared, written by whatever `launch` issues, read back with one synchronise.
template <class Launch>
static int device_flag(int* word, hipStream_t st, Launch&& launch) {
    SKF_HIP(hipMemsetAsync(word, 0, sizeof(int), st));
    launch();
    int v = 0;
    SKF_HIP(hipMemcpyAsync(&v, word, sizeof(int), hipMemcpyDeviceToHost, st));
    SKF_HIP(hipStreamSynchronize(st));
    return v;
}

// Caller-made CSR lists, checked on the device before anything gathers through them: indptr from 0 to nnz and
// non-decreasing, indices inside [0, cols) and strictly ascending within a row (known_csr_check_kernel; its only caller).
// `also` launches further checks that set the same word (the fill vectors of a SKF_REL_FILL_RANK1 relation): one verdict.
template <class Also>
static bool csr_is_canonical(const int64_t* indptr, const int* indices, int64_t rows, int64_t cols, int64_t nnz, int* flag_word,
                             hipStream_t st, Also&& also) {
    return device_flag(flag_word, st, [&] {
        hipLaunchKernelGGL(known_csr_check_kernel, dim3(wave_grid(rows)), dim3(256), 0, st, indptr, indices, rows, cols, nnz, flag_word);
        check_launch("known_csr_check");
        also();
    }) == 0;
}
static bool csr_is_canonical(const int64_t* indptr, const int* indices, int64_t rows, int64_t cols, int64_t nnz, int* flag_word,
                             hipStream_t st) {
    return csr_is_canonical(indptr, indices, rows, cols, nnz, flag_word, st, [] {});
}

// `n` counts on the device -> their exclusive prefix sum in int64 on the host -> n + 1 pointers uploaded to `dst`; returns
// the total.  A total above `cap` is returned WITHOUT the upload (the caller refuses or falls back).  `hc` / `hp` are the
// caller's, to be reused between calls -- after a synchronise: the upload reads `hp` until the stream has passed it.
static int64_t prefix_sum_upload(const int* counts, size_t n, void* dst, std::vector<int>& hc, std::vector<int64_t>& hp,
                                 hipStream_t st, int64_t cap = INT64_MAX) {
    if (hc.size() < n) hc.resize(n);
    if (hp.size() < n + 1) hp.resize(n + 1);
    SKF_HIP(hipMemcpyAsync(hc.data(), counts, n * 4, hipMemcpyDeviceToHost, st));
    SKF_HIP(hipStreamSynchronize(st));
    int64_t tot = 0;
    for (size_t k = 0; k < n; ++k) { hp[k] = tot; tot += hc[k]; }
    hp[n] = tot;
    if (tot <= cap) SKF_HIP(hipMemcpyAsync(dst, hp.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    return tot;
}

// ---- relations kept as their entries: row lists and column lists ---------------------------------------------------------

// The column side of the lists from their finished row side, r.kn_nnz entries (the column counts per (column, row part)
// are in r.KCnt already): prefix sums on the host, the transpose filled and every segment sorted by row on the device, then
// `values` launches the kernel that brings the values into the column order.  Ends the list building of the relation.
template <typename TM, class Values>
static void build_known_columns(skf_plan* p, RelState& r, std::vector<int>& hc, std::vector<int64_t>& hp, const char* what,
                                hipStream_t st, Values&& values) {
    const int64_t rows = r.nr, cols = p->types[r.col].n, tot = r.kn_nnz;
    const int pc = r.kn_pc, pr = r.kn_pr;
    const size_t nseg_c = (size_t)cols * pr;
    int* cnt = (int*)r.KCnt.ptr;
    int* fillpos = cnt + nseg_c;
    prefix_sum_upload(cnt, nseg_c, r.KcPtr.ptr, hc, hp, st);
    if (tot > 0) {
        hipLaunchKernelGGL(known_col_fill_kernel, dim3(wave_grid(rows)), dim3(256), 0, st, (const int64_t*)r.KrPtr.ptr,
                           (const int*)r.KrIdx.ptr, pc, rows, pr, r.kn_ph, (const int64_t*)r.KcPtr.ptr, fillpos, (int*)r.KcIdx.ptr);
        hipLaunchKernelGGL(csc_sort_kernel, dim3(elem_grid((int64_t)nseg_c)), dim3(256), 0, st, (const int64_t*)r.KcPtr.ptr,
                           (int*)r.KcIdx.ptr, (int64_t)nseg_c);
        values(wave_grid(cols));
        check_launch(what);
        // known entries: before the first iteration the completed relation is the known entries and zeros
        // (_dfmc.py:287-292), E = R there; a SKF_REL_SPARSE_CSR relation keeps no residuals
        if (r.KcE.ptr) SKF_HIP(hipMemcpyAsync(r.KcE.ptr, r.KcVal.ptr, (size_t)tot * sizeof(TM), hipMemcpyDeviceToDevice, st));
    }
    if (r.Sp.ptr) SKF_HIP(hipMemsetAsync(r.Sp.ptr, 0, r.Sp.bytes, st));
    if (r.FiB.bytes) SKF_HIP(hipMemsetAsync(r.FiB.ptr, 0, r.FiB.bytes, st));
    SKF_HIP(hipStreamSynchronize(st));                      // the host vectors die here
    r.R = nullptr;                                          // nothing reads the relation itself after this
}

// The known entries of a masked relation as row lists and column lists: counts per (row, column part) on the device,
// prefix sums on the host, fills on the device; the column lists are the transpose of the row lists, every (column, row
// part) segment sorted by row.  R values come from the caller's relation, which is not referenced afterwards.
template <typename TR, typename TM>
static void build_known_lists_t(skf_plan* p, RelState& r, hipStream_t st) {
    const int64_t rows = r.nr, cols = p->types[r.col].n;
    const int pc = r.kn_pc, pr = r.kn_pr;
    const int wgrid = wave_grid(rows);
    int* cnt = (int*)r.KCnt.ptr;
    hipLaunchKernelGGL(known_row_count_kernel, dim3(wgrid), dim3(256), 0, st, (const uint8_t*)r.Mb.ptr, r.ldmb, rows, cols, pc,
                       r.kn_pw, cnt);
    check_launch("known_row_count");
    const size_t nseg_r = (size_t)rows * pc, nseg_c = (size_t)cols * pr;
    std::vector<int> hc;
    std::vector<int64_t> hp;
    const int64_t tot = prefix_sum_upload(cnt, nseg_r, r.KrPtr.ptr, hc, hp, st, r.kn_cap);
    if (tot > r.kn_cap)
        SKF_FAIL(SKF_E_INVALID, "a masked relation holds %lld known entries, more than the bound %lld given in skf_relation_desc.known_bound",
                 (long long)tot, (long long)r.kn_cap);
    r.kn_nnz = tot;
    SKF_HIP(hipMemsetAsync(cnt, 0, 2 * nseg_c * 4, st));
    SKF_HIP(hipStreamSynchronize(st));                      // (`hp` is reused for the column side)
    if (tot > 0) {
        hipLaunchKernelGGL((known_row_fill_kernel<TR, TM>), dim3(wgrid), dim3(256), 0, st, (const uint8_t*)r.Mb.ptr, r.ldmb, rows, cols,
                           pc, (const int64_t*)r.KrPtr.ptr, (const TR*)r.R_in, r.ld_in, (int*)r.KrIdx.ptr, (TM*)r.KrVal.ptr);
        hipLaunchKernelGGL(known_col_count_kernel, dim3(wgrid), dim3(256), 0, st, (const int64_t*)r.KrPtr.ptr, (const int*)r.KrIdx.ptr,
                           pc, rows, pr, r.kn_ph, cnt);
        check_launch("known_row_fill");
    }
    build_known_columns<TM>(p, r, hc, hp, "known_col_fill", st, [&](int cgrid) {      // the values: a gather from the dense relation
        hipLaunchKernelGGL((known_col_values_kernel<TR, TM>), dim3(cgrid), dim3(256), 0, st, (const int64_t*)r.KcPtr.ptr,
                           (const int*)r.KcIdx.ptr, pr, cols, (const TR*)r.R_in, r.ld_in, (TM*)r.KcVal.ptr);
    });
}

// SKF_REL_FILL_RANK1: copies of the fill vectors a, b; the row lists' values v -> d = v - a_r b_c (once, before the column
// lists are built from them); the constants of the error formula in f64, every sum in ascending order: |a|^2, |b|^2 on the
// host from the copies, 2 sum d a_r b_c from the per-row sums of fill_residual_kernel.  The caller's vectors are not
// referenced afterwards.
template <typename TM>
static void bind_relation_fill(skf_plan* p, RelState& r, hipStream_t st) {
    const int64_t rows = r.nr, cols = p->types[r.col].n;
    SKF_HIP(hipMemcpyAsync(r.Fa.ptr, r.fill_row, (size_t)rows * sizeof(TM), hipMemcpyDeviceToDevice, st));
    SKF_HIP(hipMemcpyAsync(r.Fb.ptr, r.fill_col, (size_t)cols * sizeof(TM), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL((fill_residual_kernel<TM>), dim3(elem_grid(rows)), dim3(256), 0, st, (const int64_t*)r.KrPtr.ptr,
                       (const int*)r.KrIdx.ptr, r.kn_pc, rows, (const TM*)r.Fa.ptr, (const TM*)r.Fb.ptr, (TM*)r.KrVal.ptr,
                       (double*)r.Frow.ptr);
    check_launch("fill_residual");
    std::vector<TM> ha((size_t)rows), hb((size_t)cols);
    std::vector<double> hs((size_t)rows);
    SKF_HIP(hipMemcpyAsync(ha.data(), r.Fa.ptr, (size_t)rows * sizeof(TM), hipMemcpyDeviceToHost, st));
    SKF_HIP(hipMemcpyAsync(hb.data(), r.Fb.ptr, (size_t)cols * sizeof(TM), hipMemcpyDeviceToHost, st));
    SKF_HIP(hipMemcpyAsync(hs.data(), r.Frow.ptr, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
    SKF_HIP(hipStreamSynchronize(st));
    double aa = 0.0, bb = 0.0, dab = 0.0;
    for (int64_t k = 0; k < rows; ++k) { aa += (double)ha[k] * (double)ha[k]; dab += hs[k]; }
    for (int64_t k = 0; k < cols; ++k) bb += (double)hb[k] * (double)hb[k];
    r.fill_aa = aa; r.fill_bb = bb; r.fill_dab = 2.0 * dab;
    r.fill_row = r.fill_col = nullptr;
}

// The same lists from the caller's CSR (SKF_REL_KNOWN_CSR): validated on the device first -- nothing gathers through them
// before the host has read the verdict --, then the row lists are copies of the CSR with the part split points found by
// binary search, and the column side is built as above, its values taken from the row lists.  Byte for byte the lists
// build_known_lists_t makes from a dense relation + mask holding the same entries.  The stored entries of a
// SKF_REL_SPARSE_CSR relation (unstored = zero) take the same way: same validation, same lists, no residual list.
template <typename TR, typename TM>
static void build_known_lists_csr_t(skf_plan* p, RelState& r, hipStream_t st) {
    const int64_t rows = r.nr, cols = p->types[r.col].n, tot = r.kn_cap;
    const int pc = r.kn_pc, pr = r.kn_pr;
    int* cnt = (int*)r.KCnt.ptr;
    if (r.fill && !(r.fill_row && r.fill_col))
        SKF_FAIL(SKF_E_INVALID, "a SKF_REL_FILL_RANK1 relation without skf_plan_set_relation_fill");
    const bool lists_ok = csr_is_canonical(r.csr_ptr, r.csr_idx, rows, cols, tot, cnt, st, [&] {
        if (!r.fill) return;           // the fill vectors, in the validation itself: nothing is formed from a non-finite one
        hipLaunchKernelGGL((finite_check_kernel<TM>), dim3(elem_grid(rows)), dim3(256), 0, st, (const TM*)r.fill_row, rows, cnt);
        hipLaunchKernelGGL((finite_check_kernel<TM>), dim3(elem_grid(cols)), dim3(256), 0, st, (const TM*)r.fill_col, cols, cnt);
        check_launch("fill_check");
    });
    if (!lists_ok)
        SKF_FAIL(SKF_E_INVALID, "%s: the lists are not a canonical CSR of %lld x %lld with %lld entries (indptr from 0 "
                 "to the count, non-decreasing; columns in range and strictly ascending within a row)%s",
                 r.sp0 ? "SKF_REL_SPARSE_CSR" : "SKF_REL_KNOWN_CSR", (long long)rows, (long long)cols, (long long)tot,
                 r.fill ? ", or a fill vector of SKF_REL_FILL_RANK1 holds a value that is not finite" : "");
    r.kn_nnz = tot;
    hipLaunchKernelGGL(parted_ptr_kernel, dim3(elem_grid(rows * pc + 1)), dim3(256), 0, st, r.csr_ptr, r.csr_idx, rows, pc, r.kn_pw,
                       (int64_t*)r.KrPtr.ptr);
    check_launch("known_csr_rows");
    SKF_HIP(hipMemsetAsync(cnt, 0, 2 * (size_t)cols * pr * 4, st));
    if (tot > 0) {
        SKF_HIP(hipMemcpyAsync(r.KrIdx.ptr, r.csr_idx, (size_t)tot * 4, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL((known_csr_values_kernel<TR, TM>), dim3(elem_grid(tot)), dim3(256), 0, st, (const TR*)r.csr_val, tot,
                           (TM*)r.KrVal.ptr);
        hipLaunchKernelGGL(known_col_count_kernel, dim3(wave_grid(rows)), dim3(256), 0, st, (const int64_t*)r.KrPtr.ptr,
                           (const int*)r.KrIdx.ptr, pc, rows, pr, r.kn_ph, cnt);
        check_launch("known_csr_fill");
    }
    if (r.fill) bind_relation_fill<TM>(p, r, st);        // (before the column lists take their values from the row lists)
    std::vector<int> hc;
    std::vector<int64_t> hp;
    build_known_columns<TM>(p, r, hc, hp, "known_csr_cols", st, [&](int cgrid) {      // the values: looked up in the row lists
        hipLaunchKernelGGL((known_col_values_csr_kernel<TM>), dim3(cgrid), dim3(256), 0, st, (const int64_t*)r.KcPtr.ptr,
                           (const int*)r.KcIdx.ptr, pr, cols, (const int64_t*)r.KrPtr.ptr, (const int*)r.KrIdx.ptr, pc,
                           (const TM*)r.KrVal.ptr, (TM*)r.KcVal.ptr);
    });
    r.csr_ptr = nullptr; r.csr_idx = nullptr; r.csr_val = nullptr;      // not referenced after bind
}
static void build_known_lists_csr(skf_plan* p, RelState& r, hipStream_t st) {
    // (SKF_REL_SPARSE_CSR hands its values over in the master type -- SKF_BF16: f32, never rounded to bf16)
    if (p->bf16 && r.sp0) build_known_lists_csr_t<float, float>(p, r, st);
    else if (p->bf16) build_known_lists_csr_t<uint16_t, float>(p, r, st);
    else if (p->f64) build_known_lists_csr_t<double, double>(p, r, st);
    else build_known_lists_csr_t<float, float>(p, r, st);
}
static void build_known_lists(skf_plan* p, RelState& r, hipStream_t st) {
    if (p->bf16) build_known_lists_t<uint16_t, float>(p, r, st);
    else if (p->f64) build_known_lists_t<double, double>(p, r, st);
    else build_known_lists_t<float, float>(p, r, st);
}

// SKF_REL_FOLD_CSR: the caller's lists along the target, validated on the device (rows = target objects, columns = partner
// objects) before anything gathers through them, then copied as they are -- no other list is built.
static void copy_fold_lists(skf_plan* p, RelState& r, hipStream_t st) {
    if (!r.csr_ptr) SKF_FAIL(SKF_E_INVALID, "a SKF_REL_FOLD_CSR relation without skf_plan_set_known_entries");
    const bool row_side = r.row == p->target;
    const int64_t rows = p->types[p->target].n, cols = p->types[row_side ? r.col : r.row].n, tot = r.kn_cap;
    if (!csr_is_canonical(r.csr_ptr, r.csr_idx, rows, cols, tot, (int*)p->sqpart.ptr, st))     // (sqpart: a scratch word)
        SKF_FAIL(SKF_E_INVALID, "SKF_REL_FOLD_CSR: the lists are not canonical for %lld target x %lld partner objects with %lld "
                 "entries (indptr from 0 to the count, non-decreasing; indices in range and strictly ascending within a list)",
                 (long long)rows, (long long)cols, (long long)tot);
    r.kn_nnz = tot;
    SKF_HIP(hipMemcpyAsync(r.KrPtr.ptr, r.csr_ptr, ((size_t)rows + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (tot > 0) {
        SKF_HIP(hipMemcpyAsync(r.KrIdx.ptr, r.csr_idx, (size_t)tot * 4, hipMemcpyDeviceToDevice, st));
        SKF_HIP(hipMemcpyAsync(r.KrVal.ptr, r.csr_val, (size_t)tot * p->esz, hipMemcpyDeviceToDevice, st));
    }
    r.csr_ptr = nullptr; r.csr_idx = nullptr; r.csr_val = nullptr;      // not referenced after bind
}

// ---- dense masked relations ------------------------------------------------------------------------------------------------

// The mask in the engine's layout: one bit per entry, rows padded to whole 128-column tiles.  The caller's mask (bytes or
// bits) is not referenced after this.
static void pack_mask(skf_plan* p, RelState& r, hipStream_t st) {
    const int64_t rows = r.nr, cols = p->types[r.col].n;
    if (r.mask_is_bits) {
        SKF_HIP(hipMemsetAsync(r.Mb.ptr, 0, r.Mb.bytes, st));
        hipLaunchKernelGGL(copy_mask_bits_kernel, dim3(elem_grid(rows * ((cols + 7) / 8))), dim3(256), 0, st,
                           (uint8_t*)r.Mb.ptr, r.ldmb, r.mask, r.ldmask, rows, cols);
    } else {
        hipLaunchKernelGGL(pack_mask_kernel, dim3(elem_grid(rows * r.ldmb)), dim3(256), 0, st, (uint8_t*)r.Mb.ptr,
                           r.ldmb, r.mask, r.ldmask, rows, cols);
    }
    check_launch("pack_mask");
}

// SKF_BF16, dense completion: the known entries of every tile of the completion pass (256 rows x 128 columns) as a compact
// list (count, prefix sum on the host, fill).  32-bit counts and offsets, and the list is dropped when it outgrows its
// slot: a form of its own beside prefix_sum_upload.
static void build_tile_lists(skf_plan* p, RelState& r, hipStream_t st) {
    const int64_t rows = r.nr, cols = p->types[r.col].n;
    const int tx = cdiv(rows, 256), ty = cdiv(cols, 128);
    const size_t tiles = (size_t)tx * ty;
    KnownArgs ka;
    ka.mbits = (const uint8_t*)r.Mb.ptr; ka.ldmb = r.ldmb;
    ka.Rin = (const uint16_t*)r.R_in; ka.ldin = r.ld_in;
    ka.rows = (int)rows; ka.cols = (int)cols;
    ka.tile_cols = 128;
    ka.counts = (uint32_t*)r.Kcnt.ptr; ka.off = nullptr; ka.list = nullptr;
    hipLaunchKernelGGL(known_entries_kernel, dim3(tx, ty), dim3(256), 0, st, ka);
    check_launch("known_entries(count)");
    std::vector<uint32_t> cnt(tiles), off(tiles + 1);
    SKF_HIP(hipMemcpyAsync(cnt.data(), r.Kcnt.ptr, tiles * 4, hipMemcpyDeviceToHost, st));
    SKF_HIP(hipStreamSynchronize(st));
    uint64_t tot = 0;
    for (size_t t = 0; t < tiles; ++t) { off[t] = (uint32_t)tot; tot += cnt[t]; }
    off[tiles] = (uint32_t)tot;
    r.use_klist = tot <= r.kcap && tot < 0xFFFFFFFFull;
    if (!r.use_klist) return;
    SKF_HIP(hipMemcpyAsync(r.Koff.ptr, off.data(), (tiles + 1) * 4, hipMemcpyHostToDevice, st));
    ka.off = (const uint32_t*)r.Koff.ptr; ka.list = (uint32_t*)r.Klist.ptr;
    hipLaunchKernelGGL(known_entries_kernel, dim3(tx, ty), dim3(256), 0, st, ka);
    check_launch("known_entries(fill)");
    SKF_HIP(hipStreamSynchronize(st));          // `off` dies here
}

// Step 1: every relation's mask in the engine's layout and its lists, whichever way the entries came in.
static void bind_relation_lists(skf_plan* p, hipStream_t st) {
    for (RelState& r : p->rels) {
        const RelForm form = form_of(r);
        if (form == REL_FOLD || form == REL_FOLD_KNOWN) {
            copy_fold_lists(p, r, st);
            continue;
        }
        if (form == REL_STORED || r.kn_csr) {  // the caller's CSR, validated, then the same lists the mask form builds
            if (r.absent) continue;            // (row ownership, no row of the relation here: no lists, only the flag)
            if (!r.csr_ptr) SKF_FAIL(SKF_E_INVALID, "a SKF_REL_KNOWN_CSR / SKF_REL_SPARSE_CSR relation without skf_plan_set_known_entries");
            build_known_lists_csr(p, r, st);
            continue;
        }
        if (!r.mask) continue;
        pack_mask(p, r, st);
        if (form == REL_KNOWN) {               // the known entries as lists; no working copy of the relation
            build_known_lists(p, r, st);
            continue;
        }
        if (p->bf16) {                         // (the padded copy of bind_bf16_copies is the working set)
            build_tile_lists(p, r, st);
            continue;
        }
        const int64_t cols = p->types[r.col].n;
        copy2d(r.Rw.ptr, cols, r.R_in, r.ld_in, r.nr, cols, p->esz, st);
        r.R = r.Rw.ptr;
        r.ldr = cols;
    }
}

// ---- SKF_BF16: the engine's copies of the relations ----------------------------------------------------------------------

// CSR + CSC of a very sparse binary relation from its bitmap: per-row counts on the device, prefix sums on the host; kept
// only when the ones fit the slots sized at plan creation (1 entry in 256)
static void build_sparse_pattern(skf_plan* p, RelState& r, hipStream_t st) {
    r.sparse = false;
    if (r.sp_cap <= 0 || !r.SpRp.ptr) return;
    const int64_t rows = r.nr, cols = p->types[r.col].n;
    if (rows <= 0 || cols <= 0) return;
    const int wgrid = wave_grid(rows);
    int* rowcnt = (int*)r.SpCnt.ptr;
    int* colcnt = rowcnt + rows;
    int* fillpos = colcnt + cols;
    hipLaunchKernelGGL(bits_row_count_kernel, dim3(wgrid), dim3(256), 0, st, (const uint8_t*)r.Bb.ptr, r.ldbb, rows, rowcnt);
    check_launch("bits_row_count");
    // the form by the count: lists over bf16 factor rows (srp_bf16_v6_kernel<.., SRP_ONES>) up to 1 entry in 80 -- measured
    // at config 5 (profiles/r03_srp_v6.txt): ~14-22 ps per one and contraction against ~0.28 ps per CELL of the bitmap
    // kernels, break-even near 1 in 64 --; without that form (other ranks) lists over the f32 rows up to 1 in 256
    const int64_t cap = r.sp_gather ? r.sp_cap : std::min(r.sp_cap, rows * cols / 256);
    std::vector<int> cnt;
    std::vector<int64_t> ptr;
    const int64_t tot = prefix_sum_upload(rowcnt, (size_t)rows, r.SpRp.ptr, cnt, ptr, st, cap);
    if (tot > cap) return;
    r.sp_nnz = tot;
    SKF_HIP(hipMemsetAsync(colcnt, 0, (size_t)cols * 2 * 4, st));
    SKF_HIP(hipStreamSynchronize(st));                       // (`ptr` is reused below)
    if (tot > 0) {
        hipLaunchKernelGGL(bits_csr_fill_kernel, dim3(wgrid), dim3(256), 0, st, (const uint8_t*)r.Bb.ptr, r.ldbb, rows,
                           (const int64_t*)r.SpRp.ptr, (int*)r.SpCi.ptr);
        hipLaunchKernelGGL(csr_col_count_kernel, dim3(elem_grid(tot)), dim3(256), 0, st, (const int*)r.SpCi.ptr, tot, colcnt);
        check_launch("bits_csr_fill");
    }
    prefix_sum_upload(colcnt, (size_t)cols, r.SpCp.ptr, cnt, ptr, st);
    if (tot > 0) {
        hipLaunchKernelGGL(csr_transpose_fill_kernel, dim3(wgrid), dim3(256), 0, st, (const int64_t*)r.SpRp.ptr,
                           (const int*)r.SpCi.ptr, rows, (const int64_t*)r.SpCp.ptr, fillpos, (int*)r.SpRi.ptr);
        hipLaunchKernelGGL(csc_sort_kernel, dim3(elem_grid(cols)), dim3(256), 0, st, (const int64_t*)r.SpCp.ptr,
                           (int*)r.SpRi.ptr, cols);
        check_launch("csc_build");
    }
    if (r.sp_gather) {          // lists in parts pinned to XCDs, as long as a segment still holds a batch of entries
        const bool forced = p->sw.known_parts_forced;                    // (tests: short lists in parts too)
        auto fit = [&](int q, int64_t n_out) {
            while (!forced && q > 1 && (double)tot / ((double)n_out * q) < 64.0) q /= 2;
            return q;
        };
        r.sp_pc = fit(r.SpRpP.ptr ? r.sp_pc : 1, rows);
        r.sp_pr = fit(r.SpCpP.ptr ? r.sp_pr : 1, cols);
        r.sp_pw = ((cols + r.sp_pc - 1) / r.sp_pc + 63) / 64 * 64;
        r.sp_ph = ((rows + r.sp_pr - 1) / r.sp_pr + 63) / 64 * 64;
        if (r.sp_pc > 1)
            hipLaunchKernelGGL(parted_ptr_kernel, dim3(elem_grid(rows * r.sp_pc + 1)), dim3(256), 0, st, (const int64_t*)r.SpRp.ptr,
                               (const int*)r.SpCi.ptr, rows, r.sp_pc, r.sp_pw, (int64_t*)r.SpRpP.ptr);
        if (r.sp_pr > 1)
            hipLaunchKernelGGL(parted_ptr_kernel, dim3(elem_grid(cols * r.sp_pr + 1)), dim3(256), 0, st, (const int64_t*)r.SpCp.ptr,
                               (const int*)r.SpRi.ptr, cols, r.sp_pr, r.sp_ph, (int64_t*)r.SpCpP.ptr);
        check_launch("parted_ptr");
    }
    SKF_HIP(hipStreamSynchronize(st));
    r.sparse = true;
}

// Step 2 (SKF_BF16): the caller's bf16 relation is copied ONCE into a zero-padded row-major layout (rows to a multiple of
// 64: the inner dimension of Q = R^T G_i; columns to a multiple of 64: the inner dimension of P = R G_j) -- a 0/1 relation
// as a bitmap, very sparse ones as lists as well; it is not referenced after this
static void bind_bf16_copies(skf_plan* p, hipStream_t st) {
    if (!p->bf16) return;
    for (TypeState& t : p->types) {
        SKF_HIP(hipMemsetAsync(t.GTb.ptr, 0, t.GTb.bytes, st));
        if (t.Grow.bytes) SKF_HIP(hipMemsetAsync(t.Grow.ptr, 0, t.Grow.bytes, st));
    }
    for (RelState& r : p->rels) {
        if (r.absent || form_of(r) != REL_DENSE) continue;      // (the list forms keep no copy of a matrix)
        const int64_t rows = r.nr, cols = p->types[r.col].n;
        if (r.binary) {
            int* bad = (int*)p->sqpart.ptr;                  // (scratch word)
            const int hbad = device_flag(bad, st, [&] {
                hipLaunchKernelGGL(pack_binary_kernel, dim3(elem_grid(r.kq * r.ldbb)), dim3(256), 0, st, (uint8_t*)r.Bb.ptr,
                                   r.ldbb, r.kq, (const uint16_t*)r.R_in, r.ld_in, rows, cols, bad);
                check_launch("pack_binary");
            });
            if (hbad) SKF_FAIL(SKF_E_INVALID, "a relation flagged SKF_REL_BINARY holds an entry that is neither 0 nor 1");
            if (r.Hb.bytes) {
                SKF_HIP(hipMemsetAsync(r.Hb.ptr, 0, r.Hb.bytes, st));
                SKF_HIP(hipMemsetAsync(r.Gb.ptr, 0, r.Gb.bytes, st));
            }
            r.R = r.Bb.ptr;
            r.ldr = r.ldrb;
            build_sparse_pattern(p, r, st);
            continue;
        }
        SKF_HIP(hipMemsetAsync(r.Rb.ptr, 0, r.Rb.bytes, st));
        if (r.Hb.bytes) {
            SKF_HIP(hipMemsetAsync(r.Hb.ptr, 0, r.Hb.bytes, st));
            SKF_HIP(hipMemsetAsync(r.Gb.ptr, 0, r.Gb.bytes, st));
        }
        launch_to_bf16<uint16_t>((uint16_t*)r.Rb.ptr, r.ldrb, (const uint16_t*)r.R_in, r.ld_in, rows, cols, false, st);
        r.R = r.Rb.ptr;
        r.ldr = r.ldrb;
    }
}

// ---- constraints -----------------------------------------------------------------------------------------------------------

// Step 3: CSR of every sparse constraint -- per-row counts on the device, prefix sum on the host, fill on the device
// The hub rows of a sparse constraint from its row pointers on the host (`rp`, n + 1 of them): every row longer than the
// plan's threshold cut into segments of at most that many entries; the two tables uploaded, host copies kept.
static void bind_theta_hubs(ThetaState& th, const int64_t* rp, int64_t n, hipStream_t st) {
    th.n_seg = 0;
    th.hub_rows.clear();
    th.hub_first.clear();
    if (th.hub_row <= 0 || th.seg_cap <= 0) return;
    std::vector<ThetaSeg> segs;
    std::vector<ThetaHub> hubs;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t a = rp[r], b = rp[r + 1];
        if (b - a <= th.hub_row) continue;
        ThetaHub h = {(int32_t)r, (int32_t)segs.size(), 0, 0};
        for (int64_t q = a; q < b; q += th.hub_row) {
            segs.push_back(ThetaSeg{q, (int32_t)std::min<int64_t>(th.hub_row, b - q), (int32_t)r});
            ++h.count;
        }
        hubs.push_back(h);
        th.hub_rows.push_back((int)r);
        th.hub_first.push_back(h.first);
    }
    if ((int64_t)segs.size() > th.seg_cap)
        SKF_FAIL(SKF_E_STATE, "constraint on type %d: %zu hub segments, more than the %lld the plan sized its scratch for",
                 th.type, segs.size(), (long long)th.seg_cap);
    th.n_seg = (int64_t)segs.size();
    th.hub_first.push_back((int)segs.size());
    if (segs.empty()) return;
    SKF_HIP(hipMemcpyAsync(th.HubSeg.ptr, segs.data(), segs.size() * sizeof(ThetaSeg), hipMemcpyHostToDevice, st));
    SKF_HIP(hipMemcpyAsync(th.HubRows.ptr, hubs.data(), hubs.size() * sizeof(ThetaHub), hipMemcpyHostToDevice, st));
    SKF_HIP(hipStreamSynchronize(st));          // (the host vectors end here)
}

template <typename T>
static void bind_theta_csr_t(skf_plan* p, hipStream_t st) {
    std::vector<int> cnt;
    std::vector<int64_t> rp;
    for (size_t k = 0; k < p->thetas.size(); ++k) {
        ThetaState& th = p->thetas[k];
        if (!th.sparse) continue;
        const int64_t n = p->types[th.type].n;
        if (th.entries) {       // the caller's lists, validated on the device before anything gathers through them, then copied as they are
            if (!th.csr_ptr) SKF_FAIL(SKF_E_INVALID, "constraint %zu is given as its entries (data == NULL) without skf_plan_set_constraint_entries", k);
            const int64_t tot = th.nnz_cap;
            const int64_t rows = th.local ? th.ln : n;       // (local rows: the slice of the owned rows, columns over the whole type)
            if (!csr_is_canonical(th.csr_ptr, th.csr_idx, rows, n, tot, (int*)th.Cnt.ptr, st))      // (Cnt: a scratch word)
                SKF_FAIL(SKF_E_INVALID, "constraint %zu: the lists are not canonical for %lld rows of %lld objects with %lld entries (indptr "
                         "from 0 to the count, non-decreasing; indices in range and strictly ascending within a row)", k, (long long)rows,
                         (long long)n, (long long)tot);
            th.nnz = tot;
            SKF_HIP(hipMemcpyAsync(th.Rp.ptr, th.csr_ptr, ((size_t)rows + 1) * 8, hipMemcpyDeviceToDevice, st));
            if (tot > 0) {
                SKF_HIP(hipMemcpyAsync(th.Ci.ptr, th.csr_idx, (size_t)tot * 4, hipMemcpyDeviceToDevice, st));
                SKF_HIP(hipMemcpyAsync(th.Vv.ptr, th.csr_val, (size_t)tot * sizeof(T), hipMemcpyDeviceToDevice, st));
            }
            th.csr_ptr = nullptr; th.csr_idx = nullptr; th.csr_val = nullptr;      // not referenced after bind
            if (th.seg_cap > 0 && tot > 0) {        // the row pointers back on the host: which rows are hubs
                if (rp.size() < (size_t)rows + 1) rp.resize((size_t)rows + 1);
                SKF_HIP(hipMemcpyAsync(rp.data(), th.Rp.ptr, ((size_t)rows + 1) * 8, hipMemcpyDeviceToHost, st));
                SKF_HIP(hipStreamSynchronize(st));
                bind_theta_hubs(th, rp.data(), rows, st);       // (local rows: the tables carry them)
            }
            continue;
        }
        const int grid = wave_grid(n);
        hipLaunchKernelGGL((theta_row_count_kernel<T>), dim3(grid), dim3(256), 0, st, (const T*)th.data, th.ld, n, (int*)th.Cnt.ptr);
        check_launch("theta_row_count");
        const int64_t tot = prefix_sum_upload((const int*)th.Cnt.ptr, (size_t)n, th.Rp.ptr, cnt, rp, st, th.nnz_cap);
        if (tot > th.nnz_cap)
            SKF_FAIL(SKF_E_INVALID, "constraint on type %d holds %lld non-zeros, more than the bound %lld given in skf_theta_desc.nnz",
                     th.type, (long long)tot, (long long)th.nnz_cap);
        th.nnz = tot;
        hipLaunchKernelGGL((theta_csr_fill_kernel<T>), dim3(grid), dim3(256), 0, st, (const T*)th.data, th.ld, n,
                           (const int64_t*)th.Rp.ptr, (int*)th.Ci.ptr, (T*)th.Vv.ptr);
        check_launch("theta_csr_fill");
        SKF_HIP(hipStreamSynchronize(st));          // (`rp` is reused by the next constraint)
        bind_theta_hubs(th, rp.data(), n, st);      // (the row pointers are still on the host)
    }
}
static void bind_theta_csr(skf_plan* p, hipStream_t st) {
    if (p->f64) bind_theta_csr_t<double>(p, st);
    else bind_theta_csr_t<float>(p, st);
}

// Step 4: which halves of every dense constraint's +- split are non-empty (one device pass, read back here), and the bf16
// engine's copies of the non-empty halves
static void bind_theta_halves(skf_plan* p, hipStream_t st) {
    if (p->thetas.empty()) return;
    SKF_HIP(hipMemsetAsync(p->theta_flags.ptr, 0, p->theta_flags.bytes, st));
    for (size_t k = 0; k < p->thetas.size(); ++k) {
        ThetaState& th = p->thetas[k];
        if (th.sparse) continue;
        const int64_t n = p->types[th.type].n;
        int* fl = (int*)p->theta_flags.ptr + 2 * k;
        if (p->f64)
            hipLaunchKernelGGL((sign_flags_kernel<double>), dim3(elem_grid(n * n)), dim3(256), 0, st,
                               (const double*)th.data, th.ld, n, n, fl);
        else
            hipLaunchKernelGGL((sign_flags_kernel<float>), dim3(elem_grid(n * n)), dim3(256), 0, st,
                               (const float*)th.data, th.ld, n, n, fl);
        check_launch("sign_flags");
    }
    std::vector<int> flags(p->thetas.size() * 2);
    SKF_HIP(hipMemcpyAsync(flags.data(), p->theta_flags.ptr, flags.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    SKF_HIP(hipStreamSynchronize(st));
    for (size_t k = 0; k < p->thetas.size(); ++k) {
        ThetaState& th = p->thetas[k];
        if (th.sparse) continue;
        th.has_pos = flags[2 * k] != 0;
        th.has_neg = flags[2 * k + 1] != 0;
        if (!p->bf16) continue;
        const int64_t n = p->types[th.type].n;
        for (int half = 0; half < 2; ++half) {
            if (!(half == 0 ? th.has_pos : th.has_neg)) continue;
            Slot& dst = half == 0 ? th.Pb : th.Nb;
            SKF_HIP(hipMemsetAsync(dst.ptr, 0, dst.bytes, st));
            hipLaunchKernelGGL(split_to_bf16_kernel, dim3(elem_grid(n * n)), dim3(256), 0, st, (uint16_t*)dst.ptr,
                               th.ldb, (const float*)th.data, th.ld, n, n, half == 0 ? AOP_POS : AOP_NEG);
            check_launch("split_to_bf16");
        }
    }
}

// ---- tables ----------------------------------------------------------------------------------------------------------------

// Step 5: the orders (padded and true) of the Gram matrices, as the pseudo-inverse kernels read them
static void bind_pinv_tables(skf_plan* p, hipStream_t st) {
    if (p->variant == SKF_TRANSFORM) return;
    std::vector<int> n_pad, n_orig;
    for (TypeState& t : p->types) {
        n_pad.push_back(t.n_pad);
        n_orig.push_back(t.c);
    }
    SKF_HIP(hipMemcpyAsync(p->eigN.ptr, n_pad.data(), n_pad.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SKF_HIP(hipMemcpyAsync(p->eigNorig.ptr, n_orig.data(), n_orig.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SKF_HIP(hipStreamSynchronize(st));     // the host vectors die here
}

// Step 6: job tables and the pointer table of the fused small-graph schedule (skf_small.h), unless a switch turns it off
static void bind_small_tables(skf_plan* p, hipStream_t st) {
    if (p->small_fused && (p->sw.no_small_fused || p->sw.no_small_chain)) p->small_fused = false;
    if (!p->small_fused) return;
    SmTables tb;
    memset(&tb, 0, sizeof tb);
    tb.n_types = (int)p->types.size(); tb.n_rels = (int)p->rels.size(); tb.n_thetas = (int)p->thetas.size();
    tb.nan_upd = 1;                                   // DFMF: nan_to_num on the A / B / C / D terms (_dfmf.py:254-276)
    tb.wpart = (double*)p->sm_wpart.ptr; tb.gpart = (double*)p->sm_gpart.ptr;
    tb.tickets = (int*)p->sm_tickets.ptr;
    SKF_HIP(hipMemsetAsync(p->sm_tickets.ptr, 0, p->sm_tickets.bytes, st));
    tb.eigA = (double*)p->eigA.ptr; tb.eigV = (double*)p->eigV.ptr; tb.eigOk = (int*)p->eigOk.ptr;
    tb.eig_stride = p->eig_stride;
    tb.chol_thr = chol_rel_threshold(p->sw);
    tb.eig.A = (double*)p->eigA.ptr; tb.eig.V = (double*)p->eigV.ptr; tb.eig.Vs = (double*)p->eigVs.ptr;
    tb.eig.w = (double*)p->eigW.ptr; tb.eig.stride = p->eig_stride; tb.eig.wstride = p->eig_maxn;
    tb.eig.n = (const int*)p->eigN.ptr; tb.eig.n_orig = (const int*)p->eigNorig.ptr;
    tb.eig.chol_ok = (int*)p->eigOk.ptr;
    tb.eig.max_sweeps = 30;
    tb.defl_lo = deflation_lo(p->sw); tb.defl_hi = 1e-7;
    tb.lds_rank = p->eig_maxn < 64 ? p->eig_maxn : 64;          // packed r (r + 1) / 2 doubles inside the staging tiles
    tb.sweep_single = p->sw.small_sweep1 ? 1 : 0;
    int64_t goff = 0, woff = 0;
    for (size_t i = 0; i < p->types.size(); ++i) {
        TypeState& t = p->types[i];
        SmType& d = tb.t[i];
        d.G = t.G.ptr; d.E = t.E.ptr; d.D = t.D.ptr; d.Gram = (double*)t.Gram.ptr; d.K = (double*)t.K.ptr;
        d.n = t.n; d.c = t.c; d.gpart_off = goff; d.n_gjobs = (int)((t.n + SM_GROWS - 1) / SM_GROWS);
        goff += (int64_t)align_up((size_t)d.n_gjobs * t.c * t.c, 16);
        for (const ThetaState& th : p->thetas) d.has_theta = d.has_theta || th.type == (int)i;
    }
    for (size_t k = 0; k < p->rels.size(); ++k) {
        RelState& r = p->rels[k];
        SmRel& d = tb.r[k];
        d.R = r.R; d.ldr = r.ldr; d.P = r.P.ptr; d.Q = r.SmQ.ptr; d.n_qparts = r.sm_qparts; d.W = (double*)r.W.ptr; d.S = (double*)r.S.ptr;
        d.Bp = (double*)r.SmBp.ptr; d.Bn = (double*)r.SmBn.ptr; d.Dp = (double*)r.SmDp.ptr; d.Dn = (double*)r.SmDn.ptr;
        d.row = r.row; d.col = r.col; d.wpart_off = woff; d.n_pjobs = (int)((p->types[r.row].n + 63) / 64);
        woff += (int64_t)align_up((size_t)d.n_pjobs * p->types[r.row].c * p->types[r.col].c, 16);
    }
    for (size_t k = 0; k < p->thetas.size(); ++k) {
        ThetaState& th = p->thetas[k];
        tb.th[k].rp = (const int64_t*)th.Rp.ptr; tb.th[k].ci = (const int*)th.Ci.ptr; tb.th[k].vv = th.Vv.ptr;
        tb.th[k].type = th.type;
    }
    SKF_HIP(hipMemcpyAsync(p->sm_tables.ptr, &tb, sizeof tb, hipMemcpyHostToDevice, st));
    p->sm_batch_host.assign(1, p->sm_tables.ptr);
    SKF_HIP(hipMemcpyAsync(p->sm_batch.ptr, p->sm_batch_host.data(), sizeof(void*), hipMemcpyHostToDevice, st));
    SKF_HIP(hipMemcpyAsync(p->sm_jobs1.ptr, p->sm_j1.data(), p->sm_j1.size() * sizeof(SmJob), hipMemcpyHostToDevice, st));
    SKF_HIP(hipMemcpyAsync(p->sm_jobs3.ptr, p->sm_j3.data(), p->sm_j3.size() * sizeof(SmJob), hipMemcpyHostToDevice, st));
    SKF_HIP(hipStreamSynchronize(st));     // (`tb` dies here)
}

// ---- the rest --------------------------------------------------------------------------------------------------------------

// Step 7 (SKF_OPT_OWNED_ROWS): padded layouts of the exchanges -- rows past the objects of a type stay zero for good (they
// are gathered and scattered with the rest), the Gram range is summed as a whole
static void bind_owned_clears(skf_plan* p, hipStream_t st) {
    if (!p->owned) return;
    for (TypeState& t : p->types) {
        SKF_HIP(hipMemsetAsync(t.G.ptr, 0, t.G.bytes, st));
        SKF_HIP(hipMemsetAsync(t.E.ptr, 0, t.E.bytes, st));
        SKF_HIP(hipMemsetAsync(t.D.ptr, 0, t.D.bytes, st));
    }
    for (RelState& r : p->rels) SKF_HIP(hipMemsetAsync(r.Q.ptr, 0, r.Q.bytes, st));
    SKF_HIP(hipMemsetAsync((char*)p->ws_base + p->xg_off, 0, p->xg_bytes, st));
    SKF_HIP(hipMemsetAsync((char*)p->ws_base + p->xw_off, 0, p->xw_bytes, st));
}

// Step 8: the plan's own streams and events (kept over a re-bind)
static void bind_streams(skf_plan* p) {
    if (p->owned && !p->cs && !p->sw.no_overlap && p->sw.comm_stream)
        SKF_HIP(hipStreamCreateWithFlags(&p->cs, hipStreamNonBlocking));
    p->pipeline = !p->sw.no_pipeline;
    // (a plan on the three-launch schedule of small graphs issues everything on the caller's stream: no second stream to
    // create and destroy -- at ten restarts of the README graph the streams of the plans were 4 of 30 ms)
    if (p->variant == SKF_TRANSFORM || p->aux || p->small_fused || p->sw.no_overlap) return;
    // the second stream at the LOWEST priority: its launches fill what the contractions of the main stream
    // leave free instead of taking CUs from them (config 5 +0.9 %, config 3 +0.5 % against the default priority)
    int lo = 0, hi = 0;
    SKF_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    // (plans with owned rows, where the second stream carries the critical path of a rank: lowest / default /
    // highest priority measured equal -- 2.58 / 2.56 / 2.55 ms for rank 3 of 8 at config 3 --, a running
    // contraction workgroup is not preempted; profiles/r04_owned_rank_emulation.txt)
    SKF_HIP(hipStreamCreateWithPriority(&p->aux, hipStreamNonBlocking, lo));
    SKF_HIP(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    SKF_HIP(hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
    p->overlap = true;
}
