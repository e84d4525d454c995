// skf_init.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): the host side of the column-mean initialisers `random_c` / `random_vcol` on the device (reference
// _init.py:20-61; kernels and the statement of what is computed: skf_init.h), their C entry points included.  An entry
// point reads as the order of its rules:
//   SKF_E_INVALID refusals (plan, type, views, relation form) -> SKF_E_WORKSPACE refusals -> the first HIP call
//   -> the range check of the indices on the device -> the launches.
// A refused call writes no output, and leaves the scratch as it was.
//
// Covered forms of a relation (unmasked, whole, not SKF_REL_FILL_RANK1): dense in the engine's type (f64 / f32 / the padded
// bf16 copy), the bitmap of a SKF_REL_BINARY relation of SKF_BF16, the lists of a SKF_REL_SPARSE_CSR relation.  A very sparse
// 0/1 relation that SKF_BF16 keeps as lists of its ones BESIDE its bitmap is covered through the bitmap (its list kernels read
// bf16 factor rows of the widths 64 / 128 / 256 only).  Refused: everything the plan does not hold whole -- SKF_OPT_OWNED_ROWS
// plans, row blocks -- and SKF_TRANSFORM plans.
//
// The `_filled` entry points take the same forms the same way (same launches, same bits) and, beside them, the two forms of a
// relation with MISSING values (`filled`; kernels and statement: skf_init.h): INIT_KNOWN, the known-entry lists of a masked
// relation (from a mask or from the caller's CSR) over the constant the caller passes, and INIT_RANK1, entries plus rank one
// (SKF_REL_SPARSE_CSR | SKF_REL_FILL_RANK1).  A masked relation the plan keeps DENSE stays refused.

enum InitForm { INIT_DENSE, INIT_BITS, INIT_LISTS, INIT_KNOWN, INIT_RANK1 };
static bool over_fill(InitForm f) { return f == INIT_KNOWN || f == INIT_RANK1; }

// the form of relation `rel` for the two operators here, or the refusal
static InitForm init_form(const skf_plan* p, int32_t rel, const char* op, bool filled = false) {
    if (rel < 0 || rel >= (int)p->rels.size()) SKF_FAIL(SKF_E_INVALID, "%s: relation index %d out of range", op, rel);
    const RelState& r = p->rels[rel];
    if (p->variant == SKF_TRANSFORM) SKF_FAIL(SKF_E_INVALID, "%s: not for SKF_TRANSFORM plans", op);
    if (p->owned || p->sliced || r.absent || r.nr != p->types[r.row].n)
        SKF_FAIL(SKF_E_INVALID, "%s: relation %d is not held whole here (SKF_OPT_OWNED_ROWS plans and row blocks initialise on the host)", op, rel);
    const RelForm form = form_of(r);
    const bool known_lists = filled && form == REL_KNOWN;
    if (!known_lists && (r.masked || form == REL_KNOWN || r.kn_csr || r.mask))
        SKF_FAIL(SKF_E_INVALID, filled ? "%s: relation %d is masked and kept dense" : "%s: relation %d is masked / given as its known entries", op, rel);
    if (r.fill && !filled) SKF_FAIL(SKF_E_INVALID, "%s: relation %d carries a rank-one fill (SKF_REL_FILL_RANK1)", op, rel);
    switch (form) {
    case REL_FOLD: case REL_FOLD_KNOWN: SKF_FAIL(SKF_E_INVALID, "%s: relation %d is a fold-in list", op, rel);
    case REL_KNOWN: return INIT_KNOWN;
    case REL_STORED: return r.fill ? INIT_RANK1 : INIT_LISTS;
    case REL_DENSE: break;
    }
    return p->bf16 && r.binary ? INIT_BITS : INIT_DENSE;
}

// ---- line norms ----------------------------------------------------------------------------------------------------------------
// Scratch of skf_plan_relation_norms: the column partials [slabs][cols], then the row partials [column blocks][rows]
// (f64); a relation kept as lists needs none.
struct NormLayout { int64_t slabs, cblocks; size_t colpart, rowpart, total; };
static NormLayout norm_layout(int64_t rows, int64_t cols) {
    NormLayout l;
    l.slabs = (rows + NORM_ROWS - 1) / NORM_ROWS;
    l.cblocks = (cols + NORM_COLS - 1) / NORM_COLS;
    l.colpart = 0;
    l.rowpart = align_up((size_t)l.slabs * cols * 8, 256);
    l.total = l.rowpart + align_up((size_t)l.cblocks * rows * 8, 256);
    return l;
}

template <class Load>
static void launch_norms_tile(const Load& ld, int64_t rows, int64_t cols, const NormLayout& l, char* ws, double* row_sq, double* col_sq,
                              hipStream_t st) {
    double* colpart = (double*)(ws + l.colpart);
    double* rowpart = (double*)(ws + l.rowpart);
    hipLaunchKernelGGL((norms_tile_kernel<Load>), dim3((unsigned)l.slabs, (unsigned)l.cblocks), dim3(256), 0, st, ld, rows, cols, colpart, rowpart);
    check_launch("norms_tile");
    if (col_sq) hipLaunchKernelGGL(norms_final_kernel, dim3(cdiv(cols, 256)), dim3(256), 0, st, (const double*)colpart, l.slabs, cols, col_sq);
    if (row_sq) hipLaunchKernelGGL(norms_final_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, (const double*)rowpart, l.cblocks, rows, row_sq);
    check_launch("norms_final");
}

template <typename TM>
static void launch_norms_lists(const RelState& r, int64_t rows, int64_t cols, double* row_sq, double* col_sq, hipStream_t st) {
    if (row_sq)
        hipLaunchKernelGGL((norms_lists_kernel<TM>), dim3(cdiv(rows, 256)), dim3(256), 0, st, (const int64_t*)r.KrPtr.ptr, r.kn_pc,
                           (const TM*)r.KrVal.ptr, rows, row_sq);
    if (col_sq)
        hipLaunchKernelGGL((norms_lists_kernel<TM>), dim3(cdiv(cols, 256)), dim3(256), 0, st, (const int64_t*)r.KcPtr.ptr, r.kn_pr,
                           (const TM*)r.KcVal.ptr, cols, col_sq);
    check_launch("norms_lists");
}

// The lines of a relation kept as lists over a fill (INIT_KNOWN: the constant `fill`; INIT_RANK1: a b^T): rows from the row
// lists, columns from the column lists, one thread per line (norms_filled_kernel)
template <typename TM>
static void launch_norms_filled(const RelState& r, InitForm form, double fill, int64_t rows, int64_t cols, double* row_sq, double* col_sq,
                                hipStream_t st) {
    const bool rank1 = form == INIT_RANK1;
    const TM* a = rank1 ? (const TM*)r.Fa.ptr : nullptr;
    const TM* b = rank1 ? (const TM*)r.Fb.ptr : nullptr;
    if (row_sq)
        hipLaunchKernelGGL((norms_filled_kernel<TM>), dim3(cdiv(rows, 256)), dim3(256), 0, st, (const int64_t*)r.KrPtr.ptr, r.kn_pc,
                           (const int*)r.KrIdx.ptr, (const TM*)r.KrVal.ptr, rows, cols, fill, a, b, r.fill_bb, row_sq);
    if (col_sq)
        hipLaunchKernelGGL((norms_filled_kernel<TM>), dim3(cdiv(cols, 256)), dim3(256), 0, st, (const int64_t*)r.KcPtr.ptr, r.kn_pr,
                           (const int*)r.KcIdx.ptr, (const TM*)r.KcVal.ptr, cols, rows, fill, b, a, r.fill_aa, col_sq);
    check_launch("norms_filled");
}

// ---- the initialiser -----------------------------------------------------------------------------------------------------------
// One oriented view of the call: V = R (the type is the relation's row type) or R^T (its column type), n x m
struct InitView {
    const RelState* r;
    InitForm form;
    bool transposed;
    int64_t m;              // columns of the view
    int take;
    const int* sel;
    bool w_bf16;            // W in the bf16 Bt[c][ldw] layout (dense / bitmap relations of SKF_BF16), else [m][c] in the master type
    int64_t ldw;
    size_t w_bytes, part_bytes;
    double fill;            // INIT_KNOWN: the constant beneath the unknown entries
};

// Scratch of skf_plan_init_column_means: [0, 256) the flag word of the index check; W (the largest of the views); the f64
// accumulator n x c; the product of one view n x c in the master type; split-K slices / outputs of list parts (the largest)
// (views over a fill: W is their flags, one byte per (view column, factor column); they need no product, and the rank-one
// form the c column sums B at the end)
struct InitLayout { size_t w, acc, x, part, part_bytes, bk, total; };

static void init_views(const skf_plan* p, int32_t type, int32_t n_views, const skf_init_view* views, bool need_sel,
                       std::vector<InitView>& out, InitLayout& l, bool filled = false, const double* fills = nullptr) {
    const char* op = filled ? "skf_plan_init_column_means_filled" : "skf_plan_init_column_means";
    if (!p) SKF_FAIL(SKF_E_INVALID, "null plan");
    if (type < 0 || type >= (int)p->types.size()) SKF_FAIL(SKF_E_INVALID, "%s: type index %d out of range", op, type);
    if (n_views < 1 || !views) SKF_FAIL(SKF_E_INVALID, "%s: no views (a type that no relation touches has no column means)", op);
    const TypeState& t = p->types[type];
    const int c = t.c;
    size_t w_max = 0, part_max = 0;
    bool products = false, colsums = false;
    out.clear();
    for (int v = 0; v < n_views; ++v) {
        InitView iv;
        iv.form = init_form(p, views[v].rel, op, filled);
        iv.fill = 0.0;
        iv.r = &p->rels[views[v].rel];
        if (iv.r->row != type && iv.r->col != type) SKF_FAIL(SKF_E_INVALID, "%s: relation %d does not touch type %d", op, views[v].rel, type);
        iv.transposed = iv.r->col == type;
        iv.m = p->types[iv.transposed ? iv.r->row : iv.r->col].n;
        iv.take = views[v].take;
        iv.sel = (const int*)views[v].sel;
        // (fewer than 5 columns: the reference takes the mean of nothing, NaN; the host initialiser keeps that behaviour)
        if (iv.take < 1 || iv.take > iv.m) SKF_FAIL(SKF_E_INVALID, "%s: view %d averages take = %d of %lld columns", op, v, iv.take, (long long)iv.m);
        if (need_sel && !iv.sel) SKF_FAIL(SKF_E_INVALID, "%s: view %d has no index array", op, v);
        iv.w_bf16 = p->bf16 && iv.form != INIT_LISTS && !over_fill(iv.form);
        if (over_fill(iv.form)) {
            if (iv.form == INIT_KNOWN && need_sel) {
                if (!fills) SKF_FAIL(SKF_E_INVALID, "%s: view %d is a known-entry relation and no fills are given", op, v);
                if (!std::isfinite(fills[v])) SKF_FAIL(SKF_E_INVALID, "%s: the fill of view %d is not finite", op, v);
                iv.fill = fills[v];
            }
            iv.ldw = c;
            iv.w_bytes = (size_t)iv.m * c;
            iv.part_bytes = 0;
            colsums = colsums || iv.form == INIT_RANK1;
        } else if (iv.w_bf16) {
            // the inner dimension of the contraction as the relation is kept: Q = R^T .. runs over pad64(rows), P = R .. over pad64(columns)
            iv.ldw = iv.transposed ? iv.r->kq : iv.r->ldrb;
            iv.w_bytes = (size_t)c * iv.ldw * 2;
            iv.part_bytes = bf16_part_bytes((int)t.n, c, (int)iv.ldw, iv.transposed || iv.form == INIT_BITS);
        } else {
            iv.ldw = c;
            iv.w_bytes = (size_t)iv.m * c * p->esz;
            if (iv.form == INIT_LISTS) {
                const int parts = iv.transposed ? iv.r->kn_pr : iv.r->kn_pc;
                iv.part_bytes = parts > 1 ? (size_t)parts * t.n * c * p->esz : 0;
            } else {
                iv.part_bytes = kind_part_bytes(p, kind_relation(p), t.n, c, iv.m);
            }
        }
        products = products || !over_fill(iv.form);
        w_max = std::max(w_max, iv.w_bytes);
        part_max = std::max(part_max, iv.part_bytes);
        out.push_back(iv);
    }
    if (!p->bound) SKF_FAIL(SKF_E_STATE, "workspace not bound");      // (the parts of a relation's lists are settled at bind time)
    l.w = 256;
    l.acc = l.w + align_up(w_max, 256);
    l.x = l.acc + align_up((size_t)t.n * c * 8, 256);
    l.part = l.x + (products ? align_up((size_t)t.n * c * p->esz, 256) : 0);
    l.part_bytes = part_max;
    l.bk = l.part + align_up(part_max, 256);
    l.total = l.bk + (colsums ? align_up((size_t)c * 8, 256) : 0);
}

// acc += |mean| of one view kept as lists over a fill: the flags of the chosen columns, the column sums of the fill vector
// (rank one), one pass over the view's lists with the epilogue in it
template <typename TM, int NJ>
static void launch_list_means(const TypeState& t, const InitView& iv, const uint8_t* flags, const double* B, double* acc, hipStream_t st) {
    const RelState& r = *iv.r;
    const Slot& sp = iv.transposed ? r.KcPtr : r.KrPtr;
    const Slot& si = iv.transposed ? r.KcIdx : r.KrIdx;
    const Slot& sv = iv.transposed ? r.KcVal : r.KrVal;
    const TM* own = iv.form == INIT_RANK1 ? (const TM*)(iv.transposed ? r.Fb.ptr : r.Fa.ptr) : nullptr;
    hipLaunchKernelGGL((init_list_means_kernel<TM, NJ>), dim3(cdiv(t.n, 4)), dim3(256), 0, st, (const int64_t*)sp.ptr,
                       iv.transposed ? r.kn_pr : r.kn_pc, (const int*)si.ptr, (const TM*)sv.ptr, flags, t.n, t.c, iv.take, iv.fill, own,
                       iv.form == INIT_RANK1 ? B : (const double*)nullptr, acc);
    check_launch("init_list_means");
}

template <typename TM>
static void init_over_fill(const TypeState& t, const InitView& iv, uint8_t* flags, double* B, double* acc, hipStream_t st) {
    const RelState& r = *iv.r;
    SKF_HIP(hipMemsetAsync(flags, 0, iv.w_bytes, st));
    hipLaunchKernelGGL((init_sel_scatter_kernel<uint8_t>), dim3(elem_grid((int64_t)t.c * iv.take)), dim3(256), 0, st, iv.sel, t.c, iv.take,
                       flags, (int64_t)t.c, (int64_t)1, (uint8_t)1);
    check_launch("init_sel_scatter");
    if (iv.form == INIT_RANK1) {
        hipLaunchKernelGGL((init_fill_colsum_kernel<TM>), dim3(cdiv(t.c, 256)), dim3(256), 0, st, iv.sel, t.c, iv.take,
                           (const TM*)(iv.transposed ? r.Fa.ptr : r.Fb.ptr), B);
        check_launch("init_fill_colsum");
    }
    const int nj = (t.c + 63) / 64;
    if (nj <= 1) launch_list_means<TM, 1>(t, iv, flags, B, acc, st);
    else if (nj <= 2) launch_list_means<TM, 2>(t, iv, flags, B, acc, st);
    else if (nj <= 4) launch_list_means<TM, 4>(t, iv, flags, B, acc, st);
    else if (nj <= 8) launch_list_means<TM, 8>(t, iv, flags, B, acc, st);
    else if (nj <= 16) launch_list_means<TM, 16>(t, iv, flags, B, acc, st);
    else SKF_FAIL(SKF_E_INVALID, "skf_plan_init_column_means_filled: rank %d above 1024", t.c);
}

// x = V W for one view, through the contraction the plan runs for this relation and orientation (relation_gemm)
static void init_product(skf_plan* p, const TypeState& t, const InitView& iv, void* W, void* x, void* part, size_t part_bytes, hipStream_t st) {
    const RelState& r = *iv.r;
    const RelRight rhs = {W, iv.ldw, t.c, part, part_bytes};
    // (the strides of the left operand as contraction_P / contraction_Q give them; SKF_BF16 and the lists read the stored form)
    GemmArgs g = iv.transposed ? gemm_args(r.R, 1, r.ldr, W, t.c, 1, x, t.c, (int)t.n, t.c, (int)iv.m, EPI_STORE, 0)
                               : gemm_args(r.R, r.ldr, 1, W, t.c, 1, x, t.c, (int)t.n, t.c, (int)iv.m, EPI_STORE, 0);
    relation_gemm(p, g, st, &r, iv.transposed, &rhs);
}

template <typename T>
static void run_init_column_means(skf_plan* p, const TypeState& t, const std::vector<InitView>& vs, const InitLayout& l, char* ws,
                                  void* G0, int64_t ld, hipStream_t st) {
    const int64_t total = t.n * t.c;
    double* acc = (double*)(ws + l.acc);
    T* x = (T*)(ws + l.x);
    hipLaunchKernelGGL(init_acc_start_kernel, dim3(elem_grid(total)), dim3(256), 0, st, acc, total);
    check_launch("init_acc_start");
    for (const InitView& iv : vs) {
        void* W = ws + l.w;
        if (over_fill(iv.form)) {
            init_over_fill<T>(t, iv, (uint8_t*)W, (double*)(ws + l.bk), acc, st);
            continue;
        }
        SKF_HIP(hipMemsetAsync(W, 0, iv.w_bytes, st));
        const int sgrid = elem_grid((int64_t)t.c * iv.take);
        if (iv.w_bf16)
            hipLaunchKernelGGL((init_sel_scatter_kernel<uint16_t>), dim3(sgrid), dim3(256), 0, st, iv.sel, t.c, iv.take, (uint16_t*)W,
                               (int64_t)1, iv.ldw, (uint16_t)0x3F80);
        else
            hipLaunchKernelGGL((init_sel_scatter_kernel<T>), dim3(sgrid), dim3(256), 0, st, iv.sel, t.c, iv.take, (T*)W, (int64_t)t.c,
                               (int64_t)1, (T)1);
        check_launch("init_sel_scatter");
        init_product(p, t, iv, W, x, ws + l.part, l.part_bytes, st);
        hipLaunchKernelGGL((init_acc_add_kernel<T>), dim3(elem_grid(total)), dim3(256), 0, st, acc, (const T*)x, total, (double)iv.take);
        check_launch("init_acc_add");
    }
    hipLaunchKernelGGL((init_acc_store_kernel<T>), dim3(elem_grid(total)), dim3(256), 0, st, (const double*)acc, t.n, t.c, (T*)G0, ld);
    check_launch("init_acc_store");
}

// ---- the C entry points --------------------------------------------------------------------------------------------------------
// (the bodies of the entry points; `filled`: the _filled ones, which take the forms over a fill as well)
static void norms_workspace_bytes(const skf_plan* p, int32_t rel, size_t* bytes, bool filled) {
    if (!p || !bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
    const InitForm form = init_form(p, rel, filled ? "skf_plan_relation_norms_filled" : "skf_plan_relation_norms", filled);
    const RelState& r = p->rels[rel];
    *bytes = form == INIT_LISTS || over_fill(form) ? 0 : norm_layout(r.nr, p->types[r.col].n).total;
}

static void relation_norms(skf_plan* p, int32_t rel, bool filled, double fill, double* row_sq, double* col_sq, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!p) SKF_FAIL(SKF_E_INVALID, "null plan");
    const InitForm form = init_form(p, rel, filled ? "skf_plan_relation_norms_filled" : "skf_plan_relation_norms", filled);
    if (form == INIT_KNOWN && !std::isfinite(fill)) SKF_FAIL(SKF_E_INVALID, "skf_plan_relation_norms_filled: the fill is not finite");
    const RelState& r = p->rels[rel];
    const int64_t rows = r.nr, cols = p->types[r.col].n;
    const NormLayout l = norm_layout(rows, cols);
    if (l.cblocks > 65535) SKF_FAIL(SKF_E_INVALID, "skf_plan_relation_norms: more than 65535 * 256 columns");
    if (!p->bound) SKF_FAIL(SKF_E_STATE, "workspace not bound");
    if (form != INIT_LISTS && !over_fill(form)) {
        if (!workspace || workspace_bytes < l.total)
            SKF_FAIL(SKF_E_WORKSPACE, "skf_plan_relation_norms: workspace %zu B < required %zu B (or null)", workspace ? workspace_bytes : (size_t)0, l.total);
        if (((uintptr_t)workspace & 255) != 0) SKF_FAIL(SKF_E_WORKSPACE, "skf_plan_relation_norms: workspace must be 256-byte aligned");
    }
    if ((!row_sq && !col_sq) || rows == 0 || cols == 0) return;
    hipStream_t st = as_stream(stream);
    char* ws = (char*)workspace;
    if (over_fill(form)) {
        if (p->f64) launch_norms_filled<double>(r, form, fill, rows, cols, row_sq, col_sq, st);
        else launch_norms_filled<float>(r, form, fill, rows, cols, row_sq, col_sq, st);
    } else if (form == INIT_LISTS) {
        if (p->f64) launch_norms_lists<double>(r, rows, cols, row_sq, col_sq, st);
        else launch_norms_lists<float>(r, rows, cols, row_sq, col_sq, st);
    } else if (form == INIT_BITS) {
        launch_norms_tile(NormBits{(const uint8_t*)r.Bb.ptr, r.ldbb}, rows, cols, l, ws, row_sq, col_sq, st);
    } else if (p->bf16) {
        launch_norms_tile(NormDense<uint16_t>{(const uint16_t*)r.Rb.ptr, r.ldrb}, rows, cols, l, ws, row_sq, col_sq, st);
    } else if (p->f64) {
        launch_norms_tile(NormDense<double>{(const double*)r.R, r.ldr}, rows, cols, l, ws, row_sq, col_sq, st);
    } else {
        launch_norms_tile(NormDense<float>{(const float*)r.R, r.ldr}, rows, cols, l, ws, row_sq, col_sq, st);
    }
}

static void init_column_means(skf_plan* p, int32_t type, int32_t n_views, const skf_init_view* views, bool filled, const double* fills,
                              void* G0, int64_t ld, void* workspace, size_t workspace_bytes, void* stream) {
    std::vector<InitView> vs;
    InitLayout l;
    init_views(p, type, n_views, views, true, vs, l, filled, fills);
    const TypeState& t = p->types[type];
    if (!G0) SKF_FAIL(SKF_E_INVALID, "skf_plan_init_column_means: null argument");
    if (ld < t.c) SKF_FAIL(SKF_E_INVALID, "skf_plan_init_column_means: ld %lld < rank %d", (long long)ld, t.c);
    if (!p->bound) SKF_FAIL(SKF_E_STATE, "workspace not bound");
    if (!workspace || workspace_bytes < l.total)
        SKF_FAIL(SKF_E_WORKSPACE, "skf_plan_init_column_means: workspace %zu B < required %zu B (or null)", workspace ? workspace_bytes : (size_t)0, l.total);
    if (((uintptr_t)workspace & 255) != 0) SKF_FAIL(SKF_E_WORKSPACE, "skf_plan_init_column_means: workspace must be 256-byte aligned");
    if (t.n == 0) return;
    hipStream_t st = as_stream(stream);
    // every index of every view against its view's columns, before anything is written; the flag word is the first of the
    // scratch and gets its old content back when the call is refused
    int keep = 0;
    int* flag = (int*)workspace;
    SKF_HIP(hipMemcpyAsync(&keep, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    const int bad = device_flag(flag, st, [&] {
        for (const InitView& iv : vs) {
            const int64_t total = (int64_t)t.c * iv.take;
            hipLaunchKernelGGL(init_sel_check_kernel, dim3(elem_grid(total)), dim3(256), 0, st, iv.sel, total, iv.m, flag);
        }
        check_launch("init_sel_check");
    });
    if (bad) {
        SKF_HIP(hipMemcpyAsync(flag, &keep, sizeof(int), hipMemcpyHostToDevice, st));
        SKF_HIP(hipStreamSynchronize(st));
        SKF_FAIL(SKF_E_INVALID, "skf_plan_init_column_means: an index names a column outside its view");
    }
    if (p->f64) run_init_column_means<double>(p, t, vs, l, (char*)workspace, G0, ld, st);
    else run_init_column_means<float>(p, t, vs, l, (char*)workspace, G0, ld, st);
}

extern "C" {

int skf_plan_relation_norms_workspace_bytes(const skf_plan* p, int32_t rel, size_t* bytes) {
    return guarded([&] { norms_workspace_bytes(p, rel, bytes, false); });
}

int skf_plan_relation_norms(skf_plan* p, int32_t rel, double* row_sq, double* col_sq, void* workspace, size_t workspace_bytes,
                            void* stream) {
    return guarded([&] { relation_norms(p, rel, false, 0.0, row_sq, col_sq, workspace, workspace_bytes, stream); });
}

int skf_plan_relation_norms_filled_workspace_bytes(const skf_plan* p, int32_t rel, size_t* bytes) {
    return guarded([&] { norms_workspace_bytes(p, rel, bytes, true); });
}

int skf_plan_relation_norms_filled(skf_plan* p, int32_t rel, double fill, double* row_sq, double* col_sq, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    return guarded([&] { relation_norms(p, rel, true, fill, row_sq, col_sq, workspace, workspace_bytes, stream); });
}

int skf_plan_init_column_means_workspace_bytes(const skf_plan* p, int32_t type, int32_t n_views, const skf_init_view* views, size_t* bytes) {
    return guarded([&] {
        if (!bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        std::vector<InitView> vs;
        InitLayout l;
        init_views(p, type, n_views, views, false, vs, l);
        *bytes = l.total;
    });
}

int skf_plan_init_column_means(skf_plan* p, int32_t type, int32_t n_views, const skf_init_view* views, void* G0, int64_t ld,
                               void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] { init_column_means(p, type, n_views, views, false, nullptr, G0, ld, workspace, workspace_bytes, stream); });
}

int skf_plan_init_column_means_filled_workspace_bytes(const skf_plan* p, int32_t type, int32_t n_views, const skf_init_view* views,
                                                      size_t* bytes) {
    return guarded([&] {
        if (!bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        std::vector<InitView> vs;
        InitLayout l;
        init_views(p, type, n_views, views, false, vs, l, true);
        *bytes = l.total;
    });
}

int skf_plan_init_column_means_filled(skf_plan* p, int32_t type, int32_t n_views, const skf_init_view* views, const double* fills, void* G0,
                                      int64_t ld, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] { init_column_means(p, type, n_views, views, true, fills, G0, ld, workspace, workspace_bytes, stream); });
}

}  // extern "C"
