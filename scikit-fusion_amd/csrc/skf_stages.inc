// skf_stages.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): the passes over entry lists (launches around skf_known.h: known entries, stored entries, fold-in lists,
// 0/1 relations), the c x c / n x c x c algebra of DFMC on known entries around them, and the STAGED schedule of an iteration
// -- contract, backbone, accumulate, update -- which orders the steps of skf_steps.inc on one stream (the pseudo-inverses on
// a second one) and is what skf_iterate_dist cuts between its collectives.
// ------------------------------------------------------------------------------------------
// DFMC on the known entries only (skf_known.h): launches of the list passes and the c x c / n x c x c algebra around them
// ------------------------------------------------------------------------------------------
// dst = part 0 + part 1 + ... of `total` elements each (sum_parts_kernel)
template <typename T>
static void launch_sum_parts(void* dst, const void* parts, int64_t total, int nparts, hipStream_t st) {
    hipLaunchKernelGGL((sum_parts_kernel<T>), dim3(elem_grid(total)), dim3(256), 0, st, (T*)dst, (const T*)parts, total, nparts, total);
    check_launch("sum_parts");
}

// A pass over entry lists as its call site describes it: plain pointers, typed once in srp_pass below.  Every form the engine
// walks as lists -- known entries (from a mask or CSR), stored entries with or without a rank-one fill, fold-in lists, 0/1
// relations over bf16 rows -- is one of these.
struct SrpPass {
    const void* ptr;            // segment table (int64, [n_out * parts + 1]) and inner index (int) of every entry
    const void* idx;
    const void* rvals;          // value and residual lists in the list type (see bf16_rows), or none
    void* evals;
    const void* Fi;             // gathered matrix: n_in rows of leading dimension ldi
    int64_t ldi, n_in;
    const void* Fo;             // vectors of the outer objects (leading dimension ldo), or none
    int64_t ldo;
    bool bf16_rows;             // Fi / Fo are bf16 rows with an all-zero row behind row n_in of Fi, lists and sums f32;
                                // otherwise everything is of the plan's master type
    bool need_v6;               // bf16_rows: srp_bf16_kernel is no fallback when the zero row is out of the v6 kernel's reach
    void* dst;                  // [n_out][ld_out], the result (SRP_ERR: none)
    void* part;                 // [parts][n_out][w], the outputs of the parts (parts > 1)
    int64_t n_out, ld_out;
    int parts, w, mode;
    int sq_first;               // SRP_ERR: the partials go to p->sqpart from this slot on
    const void* r1_scale;       // rank-one term dst[o] += r1_scale[o] * r1_vec, added where the parts are summed, or none
    const double* r1_vec;
    int launches;               // profiling: counted launches (0: the pass is not profiled), with the caller's flop and byte
    double flops, bytes;        // formulas; prof_open: the caller recorded the opening event ahead of a step of its own
    bool prof_open;
};

// the kernel of a pass: 16-byte chunks where width, leading dimensions and bases allow, srp_any_kernel otherwise
template <typename TG, typename TM>
static void launch_srp(const SrpArgs<TG, TM>& a, hipStream_t st) {
    const int grid = (int)srp_grid(a.n_out, a.parts);
    constexpr int VE = 16 / (int)sizeof(TG);
    auto al = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
    const bool vec = a.w % VE == 0 && a.ldi % VE == 0 && al(a.Fi) && (a.mode == SRP_APPLY || (a.ldo % VE == 0 && al(a.Fo)));
    const int gl = vec ? a.w / VE : 0;
    bool done = false;
    if constexpr (std::is_same<TG, uint16_t>::value) {
        if (a.mode == SRP_ONES) {          // 0/1 relations as lists: w = 64 (8-byte chunks), 128 or 256
            if (a.w == 64) hipLaunchKernelGGL((srp_bf16_v6_kernel<1, SRP_ONES, 2>), dim3(grid), dim3(256), 0, st, a);
            else if (a.w == 128) hipLaunchKernelGGL((srp_bf16_v6_kernel<1, SRP_ONES, 4>), dim3(grid), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((srp_bf16_v6_kernel<2, SRP_ONES, 4>), dim3(grid), dim3(256), 0, st, a);
            check_launch("sparse 0/1 relation (lists)");
            return;
        }
        // srp_bf16_v6_kernel: a row of 16 lanes per gathered vector, w = 128 (both modes) or 256 (SRP_APPLY: measured, the
        // residual pass at w = 256 is faster with two rows per vector), 32-bit byte offsets, an all-zero row behind Fi
        if (a.zero_off != 0 && a.mode != SRP_ERR && (gl == 16 || (gl == 32 && a.mode == SRP_APPLY))) {
            if (gl == 16 && a.mode == SRP_RESIDUAL) hipLaunchKernelGGL((srp_bf16_v6_kernel<1, SRP_RESIDUAL>), dim3(grid), dim3(256), 0, st, a);
            else if (gl == 16) hipLaunchKernelGGL((srp_bf16_v6_kernel<1, SRP_APPLY>), dim3(grid), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((srp_bf16_v6_kernel<2, SRP_APPLY>), dim3(grid), dim3(256), 0, st, a);
            check_launch("known-entry pass (v6)");
            return;
        }
        done = true;
#define SKF_SRP_BF16(GL_)                                                                                                   \
    do {                                                                                                                    \
        if (a.mode == SRP_RESIDUAL) hipLaunchKernelGGL((srp_bf16_kernel<GL_, SRP_RESIDUAL>), dim3(grid), dim3(256), 0, st, a); \
        else if (a.mode == SRP_APPLY) hipLaunchKernelGGL((srp_bf16_kernel<GL_, SRP_APPLY>), dim3(grid), dim3(256), 0, st, a);  \
        else hipLaunchKernelGGL((srp_bf16_kernel<GL_, SRP_ERR>), dim3(grid), dim3(256), 0, st, a);                            \
    } while (0)
        if (gl == 8) SKF_SRP_BF16(8);
        else if (gl == 16) SKF_SRP_BF16(16);
        else if (gl == 32) SKF_SRP_BF16(32);
        else done = false;
#undef SKF_SRP_BF16
    }
    if (!done) {
        if (gl == 8) hipLaunchKernelGGL((srp_vec_kernel<TG, TM, 8>), dim3(grid), dim3(256), 0, st, a);
        else if (gl == 16) hipLaunchKernelGGL((srp_vec_kernel<TG, TM, 16>), dim3(grid), dim3(256), 0, st, a);
        else if (gl == 32) hipLaunchKernelGGL((srp_vec_kernel<TG, TM, 32>), dim3(grid), dim3(256), 0, st, a);
        else if (gl == 64) hipLaunchKernelGGL((srp_vec_kernel<TG, TM, 64>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((srp_any_kernel<TG, TM>), dim3(grid), dim3(256), 0, st, a);
    }
    check_launch("known-entry pass");
}

// the typed half of srp_pass: SrpArgs from the description, the kernel, then the tail that sums the parts
template <typename TG, typename TM>
static void srp_pass_typed(skf_plan* p, const SrpPass& d, uint32_t zero_off, hipStream_t st) {
    const bool parted = d.parts > 1 && d.mode != SRP_ERR;
    SrpArgs<TG, TM> a;
    memset(&a, 0, sizeof a);
    a.ptr = (const int64_t*)d.ptr; a.idx = (const int*)d.idx;
    a.rvals = (const TM*)d.rvals; a.evals = (TM*)d.evals;
    a.Fo = (const TG*)d.Fo; a.ldo = d.ldo; a.Fi = (const TG*)d.Fi; a.ldi = d.ldi;
    a.out = (TM*)(parted ? d.part : d.dst);
    a.ld_out = parted ? d.w : d.ld_out; a.part_stride = d.n_out * d.w; a.n_out = d.n_out;
    a.w = d.w; a.parts = d.parts; a.mode = d.mode;
    a.sq = (double*)p->sqpart.ptr + d.sq_first;
    a.zero_off = zero_off;
    launch_srp(a, st);
    if (d.mode == SRP_ERR) return;
    const int64_t total = d.n_out * d.w;
    if (d.r1_vec) {         // (one part: one pass over the output, in place)
        hipLaunchKernelGGL((sum_parts_rank1_kernel<TM>), dim3(elem_grid(total)), dim3(256), 0, st, (TM*)d.dst, (const TM*)a.out, total,
                           d.parts, total, d.w, (const TM*)d.r1_scale, d.r1_vec);
        check_launch("sum_parts_rank1");
    } else if (parted) {
        launch_sum_parts<TM>(d.dst, d.part, total, d.parts, st);
    }
}

// THE launcher of every list pass: capacity check of an error pass, the all-zero row of the v6 kernel, the one split over the
// gathered / list types, kernel and tail (srp_pass_typed), the profiling bracket.  Returns the waves of the pass = the error
// partials an SRP_ERR pass has written from slot d.sq_first of p->sqpart on.
static int srp_pass(skf_plan* p, const SrpPass& d, hipStream_t st) {
    const int64_t waves = srp_partials(d.n_out, d.parts);
    if (d.mode == SRP_ERR && (size_t)(waves + d.sq_first) > p->sq_elems)
        SKF_FAIL(SKF_E_STATE, "residual partials: %lld > %zu slots", (long long)(waves + d.sq_first), p->sq_elems);
    if (d.parts > 1 && d.mode != SRP_ERR && d.ld_out != d.w) SKF_FAIL(SKF_E_STATE, "list pass: strided output with parted lists");
    // slots past the end of a list point at the all-zero row behind the n_in gathered rows; byte offsets into the matrix are
    // 32 bits wide in the v6 kernel (0 = no such row within reach: srp_bf16_kernel, which needs none, or no pass at all)
    uint32_t zero_off = 0;
    if (d.bf16_rows) {
        const int64_t zoff = d.n_in * d.ldi * 2;
        if (zoff + d.ldi * 2 < (int64_t)0xffffffffLL) zero_off = (uint32_t)zoff;
        else if (d.need_v6) SKF_FAIL(SKF_E_STATE, "list pass: the gathered factor does not fit the list kernel");
    }
    const bool prof = p->profiling && d.launches > 0;
    if (prof && !d.prof_open) SKF_HIP(hipEventRecord(next_event(p), st));
    if (d.bf16_rows) srp_pass_typed<uint16_t, float>(p, d, zero_off, st);
    else if (p->f64) srp_pass_typed<double, double>(p, d, zero_off, st);
    else srp_pass_typed<float, float>(p, d, zero_off, st);
    if (prof) {
        SKF_HIP(hipEventRecord(next_event(p), st));
        p->prof_flops += d.flops;
        p->prof_bytes += d.bytes;
        p->prof_launches += d.launches;
    }
    return (int)waves;
}

// One pass over the known entries of relation r: by_col == false walks the row lists (outer = rows, gathers the rows of
// T = G_j S^T), by_col == true the column lists (outer = columns, gathers the rows of G_i).  Results land in r.A / r.Q
// (SRP_ERR: partials in p->sqpart, the number of which is returned).
static int known_pass(skf_plan* p, RelState& r, bool by_col, int mode, hipStream_t st, int sq_first = 0) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    const int ci = ti.c;
    // vectors of the row objects of the block (bf16: kept in step with G^T); rows [r0, r0 + nr) of the type under row ownership
    const void* Gi = p->bf16 ? (const void*)((const char*)ti.Grow.ptr + (size_t)r.r0 * ti.ldrow * 2)
                             : (const void*)((const char*)ti.G.ptr + (size_t)r.r0 * ci * p->esz);
    const void* Tj = p->bf16 ? r.FiB.ptr : r.Tm.ptr;          // vectors of the column objects
    const int64_t ldv = p->bf16 ? r.kn_ldf : ci;
    SrpPass d = {};
    d.ptr = by_col ? r.KcPtr.ptr : r.KrPtr.ptr;
    d.idx = by_col ? r.KcIdx.ptr : r.KrIdx.ptr;
    d.rvals = by_col ? r.KcVal.ptr : r.KrVal.ptr;
    d.evals = by_col ? r.KcE.ptr : nullptr;
    d.Fi = by_col ? Gi : Tj; d.ldi = ldv;
    d.n_in = by_col ? ti.n - r.r0 : tj.n;          // (the zero row of Grow sits behind ALL rows of the type, FiB's behind T)
    d.Fo = by_col ? Tj : Gi; d.ldo = ldv;
    d.bf16_rows = p->bf16;
    d.dst = by_col ? r.Q.ptr : r.A.ptr;
    d.part = by_col ? r.Qpart.ptr : r.Apart.ptr;
    d.n_out = by_col ? tj.n : r.nr; d.ld_out = ci;
    d.parts = by_col ? r.kn_pr : r.kn_pc; d.w = ci; d.mode = mode;
    d.sq_first = sq_first;
    d.launches = 1;
    d.flops = (mode == SRP_APPLY ? 2.0 : 4.0) * (double)r.kn_nnz * ci;
    d.bytes = (double)r.kn_nnz * (4.0 + 2.0 * p->esz);          // index + value (+ residual) lists
    return srp_pass(p, d, st);
}

// t = G^T w for SKF_REL_FILL_RANK1 (colsum_partial_kernel / colsum_final_kernel): `part` holds cdiv(n, COLSUM_ROWS) x c
// doubles, `out` c doubles.  The grid follows from n alone; 16-byte loads where width, leading dimension and base allow.
template <typename TG, typename TW>
static void launch_colsum(const TG* G, int64_t ld, int64_t n, int c, const TW* w, double* part, double* out, hipStream_t st) {
    constexpr int VE = 16 / (int)sizeof(TG);
    const int slabs = cdiv(n, COLSUM_ROWS);
    const bool vec = c % VE == 0 && ld % VE == 0 && (((uintptr_t)G) & 15) == 0;
    if (vec) hipLaunchKernelGGL((colsum_partial_kernel<TG, TW, VE>), dim3(slabs), dim3(256), 0, st, G, ld, n, c, w, part);
    else hipLaunchKernelGGL((colsum_partial_kernel<TG, TW, 1>), dim3(slabs), dim3(256), 0, st, G, ld, n, c, w, part);
    hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(c, 256)), dim3(256), 0, st, (const double*)part, (int64_t)slabs, c, out);
    check_launch("colsum");
}

// The rank-one terms of the squared error of a SKF_REL_FILL_RANK1 relation, added into slot 0 of p->sqpart (which holds the
// trace term): |a|^2 |b|^2 + 2 sum d a_r b_c - 2 (a^T G_i) S (G_j^T b).  The two sums over the objects read the MASTERS in
// every engine (the reason sparse_pass gives for its error pass); the c_i x c_j product against S is f64.
static void fill_err_terms(skf_plan* p, const RelState& r, hipStream_t st) {
    const TypeState& ti = p->types[r.row];
    const TypeState& tj = p->types[r.col];
    double* u = (double*)r.Fs.ptr;
    double* v = (double*)r.Ft.ptr;
    if (p->f64) {
        launch_colsum((const double*)ti.G.ptr, (int64_t)ti.c, ti.n, ti.c, (const double*)r.Fa.ptr, (double*)r.FpartQ.ptr, u, st);
        launch_colsum((const double*)tj.G.ptr, (int64_t)tj.c, tj.n, tj.c, (const double*)r.Fb.ptr, (double*)r.FpartP.ptr, v, st);
    } else {
        launch_colsum((const float*)ti.G.ptr, (int64_t)ti.c, ti.n, ti.c, (const float*)r.Fa.ptr, (double*)r.FpartQ.ptr, u, st);
        launch_colsum((const float*)tj.G.ptr, (int64_t)tj.c, tj.n, tj.c, (const float*)r.Fb.ptr, (double*)r.FpartP.ptr, v, st);
    }
    hipLaunchKernelGGL(fill_err_terms_kernel, dim3(1), dim3(256), 0, st, (const double*)u, (const double*)r.S.ptr, (const double*)v,
                       ti.c, tj.c, r.fill_aa * r.fill_bb + r.fill_dab, (double*)p->sqpart.ptr);
    check_launch("fill_err_terms");
}

// One pass over the stored entries of a SKF_REL_SPARSE_CSR relation (every entry not stored is zero; reference: the dense
// products of _dfmf.py:249-276 and the error of _dfmf.py:306-316):
//   err == false, is_q == false   P = R G_j    over the row lists, gathering rows of G_j   (SRP_APPLY, e = the stored value)
//   err == false, is_q == true    Q = R^T G_i  over the column lists, gathering rows of G_i
//   err == true                   sum over the row lists of (r - x)^2 - x^2, x = <(G_i S)[row], G_j[col]>: SRP_ERR with the
//                                 stored values as residuals as well ((r - e - x) = -x exactly); r.H = G_i S must be
//                                 current; one f64 partial per wave from slot `sq_first` of p->sqpart, count returned
// SKF_BF16: f32 values, bf16 factor rows (TypeState::Grow), f32 sums; f32 / f64: the master factors themselves.  The error pass
// of SKF_BF16 gathers the f32 masters too: |R|^2 - 2 <R, X> is a sum of same-signed terms r x over the stored entries that
// has to cancel against the exact trace term, so bf16 roundings of x (2^-9 each, not averaged out by differing signs as in
// a sum of squared residuals) would show in the error at 4e-4 relative; the pass is not on the hot path.
// `rhs` (RelRight, skf_plan.inc; err == false, no rank-one fill): the gathered rows are the caller's [n_in][rhs->ld] matrix
// in the master type in EVERY engine, rhs->n wide, and the outputs of the parts go to the caller's scratch.
static int sparse_pass(skf_plan* p, const RelState& r, bool is_q, bool err, void* dst, hipStream_t st, int sq_first,
                       const RelRight* rhs) {
    const TypeState& ti = p->types[r.row];
    const TypeState& tj = p->types[r.col];
    const TypeState& tin = is_q ? ti : tj;                   // the gathered factor
    const int64_t n_out = is_q ? tj.n : r.nr;
    const int parts = is_q ? r.kn_pr : r.kn_pc;
    const int w = rhs ? rhs->n : tin.c;
    if (rhs && (err || r.fill)) SKF_FAIL(SKF_E_STATE, "SKF_REL_SPARSE_CSR relation: a right operand of the caller's in an error pass / with a rank-one fill");
    if (rhs && parts > 1 && rhs->part_bytes < (size_t)parts * n_out * w * p->esz)
        SKF_FAIL(SKF_E_STATE, "SKF_REL_SPARSE_CSR relation: the caller's scratch does not hold the outputs of the list parts");
    // Q gathers rows of G_i through column lists whose indices are LOCAL rows: the gathered base is the first row of the
    // block (row ownership: the owned rows; a whole relation: row 0)
    const int64_t in0 = is_q ? r.r0 : 0;
    const bool bf16_rows = p->bf16 && !err && !rhs;
    SrpPass d = {};
    d.ptr = is_q ? r.KcPtr.ptr : r.KrPtr.ptr;
    d.idx = is_q ? r.KcIdx.ptr : r.KrIdx.ptr;
    d.rvals = is_q ? r.KcVal.ptr : r.KrVal.ptr;
    d.evals = const_cast<void*>(d.rvals);                    // (never written: SRP_APPLY / SRP_ERR only read the residual list)
    // the all-zero row of the bf16 rows sits behind ALL rows of the type, counted from the gathered base
    d.Fi = bf16_rows ? (const void*)((const uint16_t*)tin.Grow.ptr + in0 * tin.ldrow) : rows_of(p, tin.G, tin, in0);
    d.ldi = bf16_rows ? tin.ldrow : w; d.n_in = tin.n - in0;
    d.Fo = bf16_rows ? nullptr : r.H.ptr; d.ldo = d.ldi;
    d.bf16_rows = bf16_rows;
    if (rhs) { d.Fi = (const char*)rhs->B + (size_t)in0 * rhs->ld * p->esz; d.ldi = rhs->ld; d.ldo = d.ldi; }
    d.dst = dst;
    d.part = rhs ? rhs->part : (is_q ? r.Qpart.ptr : r.Apart.ptr);
    d.n_out = n_out; d.ld_out = w;
    d.parts = parts; d.w = w; d.mode = err ? SRP_ERR : SRP_APPLY;
    d.sq_first = sq_first;
    // what the pass executes and reads: index + value lists, one gathered factor row per entry (include/skfusion_hip.h)
    d.launches = 1;
    d.flops = 2.0 * (double)r.kn_nnz * w;
    d.bytes = (double)r.kn_nnz * (4.0 + (double)p->esz + (double)w * (p->bf16 ? 2.0 : (double)p->esz));
    // SKF_REL_FILL_RANK1: the weighted column sum of the gathered factor -- t = G_j^T b for P, s = G_i^T a for Q -- over the
    // rows the list pass gathers, before the lists are walked, on this stream; P[r] += a_r t / Q[c] += b_c s is added where
    // the parts are summed
    if (r.fill && !err) {
        double* tvec = (double*)(is_q ? r.Fs.ptr : r.Ft.ptr);
        double* part = (double*)(is_q ? r.FpartQ.ptr : r.FpartP.ptr);
        const void* wts = is_q ? r.Fa.ptr : r.Fb.ptr;
        if (p->profiling) SKF_HIP(hipEventRecord(next_event(p), st));
        if (p->f64) launch_colsum((const double*)tin.G.ptr, (int64_t)w, tin.n, w, (const double*)wts, part, tvec, st);
        else if (p->bf16) launch_colsum((const uint16_t*)tin.Grow.ptr, tin.ldrow, tin.n, w, (const float*)wts, part, tvec, st);
        else launch_colsum((const float*)tin.G.ptr, (int64_t)w, tin.n, w, (const float*)wts, part, tvec, st);
        d.r1_scale = is_q ? r.Fb.ptr : r.Fa.ptr;
        d.r1_vec = tvec;
        // the rank-one side (one more counted launch: the column sum with its reduce): 2 n_in w flops for the sum, 2 n_out w
        // for the term; the gathered factor and its weights once, the scale vector once, and -- lists in one part -- the
        // output read and written once more
        d.prof_open = true;
        d.launches = 2;
        d.flops += 2.0 * (double)tin.n * w + 2.0 * (double)n_out * w;
        d.bytes += (double)tin.n * ((double)w * (p->bf16 ? 2.0 : (double)p->esz) + (double)p->esz) + (double)n_out * (double)p->esz +
                   (parts > 1 ? 0.0 : 2.0 * (double)n_out * w * (double)p->esz);
    }
    return srp_pass(p, d, st);
}

// P = R G_j / Q = R^T G_i of a sparse 0/1 relation of SKF_BF16 kept as lists (RelState::sp_gather): the ones as lists over
// the bf16 rows of the gathered factor, every entry counting 1 (SRP_ONES); dst is n_out x w with leading dimension ld_out
static void ones_pass(skf_plan* p, const RelState& r, bool is_q, void* dst, int64_t ld_out, int64_t n_out, int w, hipStream_t st) {
    const TypeState& tin = p->types[is_q ? r.row : r.col];           // Q = R^T G_i sums rows of G_i, P = R G_j rows of G_j
    const int64_t in0 = is_q ? r.r0 : 0;
    if (tin.ldrow != w) SKF_FAIL(SKF_E_STATE, "sparse 0/1 relation: the gathered factor does not fit the list kernel");
    SrpPass d = {};
    d.parts = is_q ? r.sp_pr : r.sp_pc;
    d.ptr = d.parts > 1 ? (is_q ? r.SpCpP.ptr : r.SpRpP.ptr) : (is_q ? r.SpCp.ptr : r.SpRp.ptr);
    d.idx = is_q ? r.SpRi.ptr : r.SpCi.ptr;
    d.Fi = (const uint16_t*)tin.Grow.ptr + in0 * tin.ldrow; d.ldi = tin.ldrow; d.n_in = tin.n - in0;
    d.ldo = tin.ldrow;
    d.bf16_rows = true; d.need_v6 = true;
    d.dst = dst; d.part = p->sp_part.ptr;
    d.n_out = n_out; d.ld_out = ld_out; d.w = w; d.mode = SRP_ONES;
    d.launches = 1;
    d.flops = 2.0 * (double)r.sp_nnz * (double)w;
    d.bytes = 4.0 * (double)r.sp_nnz;
    srp_pass(p, d, st);
}

// ------------------------------------------------------------------------------------------
// Fold-in through a sparse relation (SKF_REL_FOLD_CSR, fold_lists_kernel in skf_known.h)
// ------------------------------------------------------------------------------------------
template <typename T>
static void launch_fold_lists(const int64_t* ptr, const int* idx, const void* val, int64_t n_out, const void* Tm, int64_t ldt, int c,
                              void* Ec, int64_t lde, void* Dc, int64_t ldd, hipStream_t st) {
    if (n_out <= 0 || c <= 0) return;
    FoldListArgs<T> a;
    a.ptr = ptr; a.idx = idx; a.val = (const T*)val; a.Tm = (const T*)Tm; a.Ec = (T*)Ec; a.Dc = (T*)Dc;
    a.n_out = n_out; a.ldt = ldt; a.lde = lde; a.ldd = ldd; a.c = c;
    int lanes = 1;
    while (lanes < 64 && lanes < c) lanes *= 2;
    a.lanes = lanes;
    const int64_t per = 256 / lanes;
    const dim3 grid((unsigned)((n_out + per - 1) / per), c > 64 ? (unsigned)cdiv(c, 256) : 1u);
    // c <= 64: one column per lane, 8 rows in flight per lane group; wider: 4 columns per lane, 4 x 4 gathers in flight
    if (c <= 64) hipLaunchKernelGGL((fold_lists_kernel<T, 1, 8>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((fold_lists_kernel<T, 4, 4>), grid, dim3(256), 0, st, a);
    check_launch("fold_lists");
}

// T of a fold-in relation given as lists: G_p S^T (the target is the row type, _dfmf.py:394-398) or G_p S (column type,
// _dfmf.py:408-412), n_partner x c_target in the master type
static void fold_form_t(skf_plan* p, RelState& r, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    const int ci = ti.c, cj = tj.c;
    GemmArgs g = r.row == p->target ? gemm_args(tj.G.ptr, cj, 1, r.S.ptr, 1, cj, r.Tm.ptr, ci, (int)tj.n, ci, cj, EPI_STORE, 0)      // G_j S^T
                                    : gemm_args(ti.G.ptr, ci, 1, r.S.ptr, cj, 1, r.Tm.ptr, cj, (int)ti.n, cj, ci, EPI_STORE, 0);     // G_i S
    mixed_gemm(p, g, st);
}

// The constant sums of prepare_transform for a SKF_REL_FOLD_CSR relation: T = G_p S^T (the target is the row type,
// _dfmf.py:394-398) or G_p S (column type, _dfmf.py:408-412) in the master type, then one pass over the lists into Ec / Dc.
// Several relations of a plan accumulate by plain read-modify-write in relation order on the one stream.
static void fold_prepare(skf_plan* p, RelState& r, hipStream_t st) {
    TypeState& tt = p->types[p->target];
    fold_form_t(p, r, st);
    if (p->f64)
        launch_fold_lists<double>((const int64_t*)r.KrPtr.ptr, (const int*)r.KrIdx.ptr, r.KrVal.ptr, tt.n, r.Tm.ptr, tt.c, tt.c,
                                  tt.Ec.ptr, tt.c, tt.Dc.ptr, tt.c, st);
    else
        launch_fold_lists<float>((const int64_t*)r.KrPtr.ptr, (const int*)r.KrIdx.ptr, r.KrVal.ptr, tt.n, r.Tm.ptr, tt.c, tt.c,
                                 tt.Ec.ptr, tt.c, tt.Dc.ptr, tt.c, st);
}

// The list part of skf_relation_sqerr for such a relation: sum over the stored entries of (r - x)^2 - x^2 with
// x = <H[o], G_p[idx]> -- the SRP_ERR launch of the fit's error pass (sparse_pass) pointed at the workspace copy of the
// lists, parts = 1, the stored values as residuals as well; r.H must be current.  Master rows in every engine (the reason
// sparse_pass gives).  One f64 partial per wave from slot `sq_first` of p->sqpart; their number is returned.
static int fold_err_pass(skf_plan* p, const RelState& r, hipStream_t st, int sq_first) {
    const bool row_side = r.row == p->target;
    const TypeState& tp = p->types[row_side ? r.col : r.row];          // the partner: its factor rows are gathered
    SrpPass d = {};
    d.ptr = r.KrPtr.ptr; d.idx = r.KrIdx.ptr;
    d.rvals = r.KrVal.ptr; d.evals = r.KrVal.ptr;            // (never written: SRP_ERR only reads the residual list)
    d.Fi = tp.G.ptr; d.ldi = tp.c; d.n_in = tp.n;
    d.Fo = r.H.ptr; d.ldo = tp.c;
    d.n_out = p->types[p->target].n; d.ld_out = tp.c;
    d.parts = 1; d.w = tp.c; d.mode = SRP_ERR;
    d.sq_first = sq_first;
    return srp_pass(p, d, st);
}

// ------------------------------------------------------------------------------------------
// Fold-in on the known entries only (SKF_REL_FOLD_KNOWN, fold_known_kernel in skf_known.h)
// ------------------------------------------------------------------------------------------
// Workgroups of the pass over n_out objects of width c: 256 / lanes objects each; an error pass writes 4 partials per
// workgroup -- at most srp_partials(n_out, 1), what plan_layout reserves for a fold-in relation.
static int fold_known_lanes(int c) {
    int lanes = 1;
    while (lanes < 64 && lanes < c) lanes *= 2;
    return lanes;
}
static int64_t fold_known_grid(int64_t n_out, int c) {
    const int64_t per = 256 / fold_known_lanes(c);
    return (n_out + per - 1) / per;
}
// sq == nullptr: E / D += the split of X + sum (v - x) T; otherwise the error partials (their number is returned)
template <typename T>
static int launch_fold_known(const int64_t* ptr, const int* idx, const void* val, int64_t n_out, const void* G, int64_t ldg,
                             const void* Tm, int64_t ldt, int c, const void* X, int64_t ldx, void* E, int64_t lde, void* D,
                             int64_t ldd, double* sq, hipStream_t st) {
    if (n_out <= 0 || c <= 0) return 0;
    FoldKnownArgs<T> a;
    a.ptr = ptr; a.idx = idx; a.val = (const T*)val; a.G = (const T*)G; a.Tm = (const T*)Tm; a.X = (const T*)X;
    a.E = (T*)E; a.D = (T*)D; a.sq = sq;
    a.n_out = n_out; a.ldg = ldg; a.ldt = ldt; a.ldx = ldx; a.lde = lde; a.ldd = ldd; a.c = c;
    a.lanes = fold_known_lanes(c);
    const dim3 grid((unsigned)fold_known_grid(n_out, c));
    // entries in flight per width class (columns per lane x entries = gathers per lane; no scratch in any instantiation)
#define SKF_FOLD_KNOWN(CPL, U)                                                                             \
    do {                                                                                                   \
        if (sq) hipLaunchKernelGGL((fold_known_kernel<T, CPL, U, true>), grid, dim3(256), 0, st, a);       \
        else hipLaunchKernelGGL((fold_known_kernel<T, CPL, U, false>), grid, dim3(256), 0, st, a);         \
    } while (0)
    if (c <= 64) SKF_FOLD_KNOWN(1, 8);
    else if (c <= 128) SKF_FOLD_KNOWN(2, 4);
    else if (c <= 256) SKF_FOLD_KNOWN(4, 4);
    else if (c <= 512) SKF_FOLD_KNOWN(8, 2);
    else SKF_FOLD_KNOWN(16, 2);
#undef SKF_FOLD_KNOWN
    check_launch("fold_known");
    return (int)grid.x * 4;
}

// Preparation of a SKF_REL_FOLD_KNOWN relation: T, and the UNSPLIT B_r = S Gram_p S^T (row side) / S^T Gram_p S (column
// side), c_t x c_t f64 like every c x c matrix of a plan, from the first product relation_small_terms left in r.U.  Nothing
// goes into Ec / Dc: nothing about this relation is constant there.
static void fold_known_prepare(skf_plan* p, RelState& r, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    const int ci = ti.c, cj = tj.c;
    fold_form_t(p, r, st);
    GemmArgs g = r.row == p->target ? gemm_args(r.U.ptr, cj, 1, r.S.ptr, 1, cj, r.Bf.ptr, ci, ci, ci, cj, EPI_STORE, 0)      // (S Gram_j) S^T
                                    : gemm_args(r.S.ptr, 1, cj, r.U.ptr, cj, 1, r.Bf.ptr, cj, cj, cj, ci, EPI_STORE, 0);     // S^T (Gram_i S)
    small_gemm(p, g, st);
}

// One iteration's share of such a relation: X = G B_r into the plan's n_t x c scratch, then E / D += the split of
// tmp1 = X + sum over the known entries of (v - <G[o], T[i]>) T[i]   (masters in every engine: SKF_BF16 runs it in f32)
static void fold_known_step(skf_plan* p, RelState& r, hipStream_t st) {
    TypeState& tt = p->types[p->target];
    const int c = tt.c;
    GemmArgs g = gemm_args(tt.G.ptr, c, 1, r.Bf.ptr, c, 1, p->fold_x.ptr, c, (int)tt.n, c, c, EPI_STORE, 0);
    mixed_gemm(p, g, st);
    if (p->f64)
        launch_fold_known<double>((const int64_t*)r.KrPtr.ptr, (const int*)r.KrIdx.ptr, r.KrVal.ptr, tt.n, tt.G.ptr, c, r.Tm.ptr, c, c,
                                  p->fold_x.ptr, c, tt.E.ptr, c, tt.D.ptr, c, nullptr, st);
    else
        launch_fold_known<float>((const int64_t*)r.KrPtr.ptr, (const int*)r.KrIdx.ptr, r.KrVal.ptr, tt.n, tt.G.ptr, c, r.Tm.ptr, c, c,
                                 p->fold_x.ptr, c, tt.E.ptr, c, tt.D.ptr, c, nullptr, st);
}

// skf_relation_sqerr of such a relation: sum over the KNOWN entries of (v - x)^2, x = <G_t[o], T[i]> with the current target
// factor; T is formed here (the preparation may not have run, or a backbone may have changed since).  One f64 partial per
// wave from slot `sq_first` of p->sqpart; their number is returned.
static int fold_known_err_pass(skf_plan* p, RelState& r, hipStream_t st, int sq_first) {
    TypeState& tt = p->types[p->target];
    const int c = tt.c;
    const int64_t waves = fold_known_grid(tt.n, c) * 4;
    if ((size_t)(waves + sq_first) > p->sq_elems)
        SKF_FAIL(SKF_E_STATE, "residual partials: %lld > %zu slots", (long long)(waves + sq_first), p->sq_elems);
    fold_form_t(p, r, st);
    double* sq = (double*)p->sqpart.ptr + sq_first;
    if (p->f64)
        return launch_fold_known<double>((const int64_t*)r.KrPtr.ptr, (const int*)r.KrIdx.ptr, r.KrVal.ptr, tt.n, tt.G.ptr, c, r.Tm.ptr,
                                         c, c, nullptr, 0, nullptr, 0, nullptr, 0, sq, st);
    return launch_fold_known<float>((const int64_t*)r.KrPtr.ptr, (const int*)r.KrIdx.ptr, r.KrVal.ptr, tt.n, tt.G.ptr, c, r.Tm.ptr, c,
                                    c, nullptr, 0, nullptr, 0, nullptr, 0, sq, st);
}

// W = G_i^T R_c G_j for the backbone (_dfmc.py:311-314) with R_c = G_i,prev S_prev G_j,prev^T + E_prev:
//     W = (G_i^T G_i,prev) S_prev (G_j,prev^T G_j) + (E_prev^T G_i)^T G_j
// first iteration: R_c = the known entries, zeros elsewhere (_dfmc.py:287-292), i.e. E_prev = R on the lists, S_prev = 0
// the two cross-Gram matrices of W: Xi = G_i^T G_i,prev, Xj = G_j,prev^T G_j (f64 accumulation over the objects)
static void known_cross(skf_plan* p, RelState& r, hipStream_t st) {
    if (p->kn_first) return;
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    const int ci = ti.c, cj = tj.c;
    // (over the rows of the block: under row ownership the block's own share of W, summed over the processes with the rest)
    GemmArgs g = gemm_args(rows_of(p, ti.G, ti, r.r0), 1, ci, rows_of(p, ti.Gp, ti, r.r0), ci, 1, r.Xi.ptr, ci, ci, ci, (int)r.nr,
                           EPI_STORE, 0);                                                                         // Xi = G_i^T G_i,prev
    wide_gemm(p, g, st);
    g = gemm_args(tj.Gp.ptr, 1, cj, tj.G.ptr, cj, 1, r.Xj.ptr, cj, cj, cj, (int)tj.n, EPI_STORE, 0);             // Xj = G_j,prev^T G_j
    wide_gemm(p, g, st);
}
static void known_w(skf_plan* p, RelState& r, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    const int ci = ti.c, cj = tj.c;
    known_pass(p, r, true, SRP_APPLY, st);                                                          // Y = E_prev^T G_i  -> r.Q
    GemmArgs g = gemm_args(r.Q.ptr, 1, ci, tj.G.ptr, cj, 1, r.W.ptr, cj, ci, cj, (int)tj.n, EPI_STORE, 0);
    wide_gemm(p, g, st);                                                                // W = Y^T G_j
    if (p->kn_first) return;
    known_cross(p, r, st);
    g = gemm_args(r.Sp.ptr, cj, 1, r.Xj.ptr, cj, 1, r.U.ptr, cj, ci, cj, cj, EPI_STORE, 0);             // U = S_prev Xj
    small_gemm(p, g, st);
    g = gemm_args(r.Xi.ptr, ci, 1, r.U.ptr, cj, 1, r.W.ptr, cj, ci, cj, ci, EPI_ACC, 0);                // W += Xi U
    small_gemm(p, g, st);
}

// behind the backbone S: the gathered vectors T = G_j S^T and the c x c operands of the dense parts
//     U2 = S^T Gram_i (Q = G_j U2 + E^T G_i) ,  Bf = S Gram_j S^T (P S^T = G_i Bf + E T)
static void known_operands(skf_plan* p, RelState& r, hipStream_t st, bool second_stream) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    const int ci = ti.c, cj = tj.c;
    GemmArgs g = gemm_args(tj.G.ptr, cj, 1, r.S.ptr, 1, cj, r.Tm.ptr, ci, (int)tj.n, ci, cj, EPI_STORE, 0);
    if (second_stream) mixed_gemm_unsplit(p, g, st);
    else mixed_gemm(p, g, st);
    if (p->bf16) launch_to_bf16<float>((uint16_t*)r.FiB.ptr, r.kn_ldf, (const float*)r.Tm.ptr, (int64_t)ci, tj.n, ci, false, st);
    g = gemm_args(r.S.ptr, 1, cj, ti.Gram.ptr, ci, 1, r.U2.ptr, ci, cj, ci, ci, EPI_STORE, 0);           // U2 = S^T Gram_i
    GemmArgs h = gemm_args(r.S.ptr, cj, 1, tj.Gram.ptr, cj, 1, r.T1.ptr, cj, ci, cj, cj, EPI_STORE, 0);    // T1 = S Gram_j
    run_gemm_pair_f64(p->engine, g, h, st, !p->sw.no_pairs);                                            // (independent: one launch)
    g = gemm_args(r.T1.ptr, cj, 1, r.S.ptr, 1, cj, r.Bf.ptr, ci, ci, ci, cj, EPI_STORE, 0);
    small_gemm(p, g, st);
}

// the two residual passes of the factor update: r.A = E T (row lists), r.Q = E^T G_i + G_j U2 (column lists; the
// residuals of this iteration replace the stored ones), and S_prev <- S
static void known_row_pass(skf_plan* p, RelState& r, hipStream_t st) { known_pass(p, r, false, SRP_RESIDUAL, st); }
// the dense part of Q on the rows [j0, j0 + nj) of the column type: Q += G_j (S^T Gram_i)
static void known_col_dense(skf_plan* p, RelState& r, int64_t j0, int64_t nj, hipStream_t st, bool second_stream) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    const int ci = ti.c, cj = tj.c;
    if (nj <= 0) return;
    GemmArgs g = gemm_args(rows_of(p, tj.G, tj, j0), cj, 1, r.U2.ptr, ci, 1, (char*)r.Q.ptr + (size_t)j0 * ci * p->esz, ci, (int)nj, ci,
                           cj, EPI_ACC, 0);
    if (second_stream) mixed_gemm_unsplit(p, g, st);
    else mixed_gemm(p, g, st);
}
static void known_col_pass(skf_plan* p, RelState& r, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    known_pass(p, r, true, SRP_RESIDUAL, st);
    known_col_dense(p, r, 0, tj.n, st, false);
    copy2d(r.Sp.ptr, tj.c, r.S.ptr, tj.c, ti.c, tj.c, 8, st);
}

// row side of the factor update from the row-side product itself: A = G_i Bf + E T, E_i (+)= A+, D_i (+)= A-
static void known_row_dense(skf_plan* p, RelState& r, hipStream_t st, bool second_stream) {
    TypeState& ti = p->types[r.row];
    const int ci = ti.c;
    GemmArgs g = gemm_args(rows_of(p, ti.G, ti, r.r0), ci, 1, r.Bf.ptr, ci, 1, r.A.ptr, ci, (int)r.nr, ci, ci, EPI_ACC, 0);
    if (second_stream) mixed_gemm_unsplit(p, g, st);
    else mixed_gemm(p, g, st);
}
static void known_row_split(skf_plan* p, RelState& r, bool accumulate, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    const int ci = ti.c;
    const int64_t total = r.nr * ci;
    if (p->f64)
        hipLaunchKernelGGL((split_accumulate_kernel<double>), dim3(elem_grid(total)), dim3(256), 0, st,
                           (double*)rows_of(p, ti.E, ti, r.r0), (double*)rows_of(p, ti.D, ti, r.r0), (const double*)r.A.ptr, total,
                           accumulate ? 1 : 0);
    else
        hipLaunchKernelGGL((split_accumulate_kernel<float>), dim3(elem_grid(total)), dim3(256), 0, st,
                           (float*)rows_of(p, ti.E, ti, r.r0), (float*)rows_of(p, ti.D, ti, r.r0), (const float*)r.A.ptr, total,
                           accumulate ? 1 : 0);
    check_launch("split_accumulate");
}
static void known_row_side(skf_plan* p, RelState& r, bool accumulate, hipStream_t st, bool second_stream) {
    known_row_dense(p, r, st, second_stream);
    known_row_split(p, r, accumulate, st);
}

// DFMC, first iteration: the unknown entries of every masked relation start at zero (_dfmc.py:287-292)
static void zero_unknown_entries(skf_plan* p, hipStream_t st) {
    for (RelState& r : p->rels) {
        if (!r.mask || r.kn) continue;          // (a known-entries relation starts from E = R on its lists, S_prev = 0)
        const int64_t rows = r.nr, cols = p->types[r.col].n;
        if (p->bf16)
            hipLaunchKernelGGL((mask_zero_kernel<uint16_t>), dim3(elem_grid(rows * cols)), dim3(256), 0, st,
                               (uint16_t*)r.Rb.ptr, r.ldrb, (const uint8_t*)r.Mb.ptr, r.ldmb, rows, cols);
        else if (p->f64)
            hipLaunchKernelGGL((mask_zero_kernel<double>), dim3(elem_grid(rows * cols)), dim3(256), 0, st,
                               (double*)r.Rw.ptr, r.ldr, (const uint8_t*)r.Mb.ptr, r.ldmb, rows, cols);
        else
            hipLaunchKernelGGL((mask_zero_kernel<float>), dim3(elem_grid(rows * cols)), dim3(256), 0, st,
                               (float*)r.Rw.ptr, r.ldr, (const uint8_t*)r.Mb.ptr, r.ldmb, rows, cols);
        check_launch("mask_zero");
    }
}

// Stage 1 of an iteration (SKF_STAGE_CONTRACT): everything that depends on G only.
static void stage_contract(skf_plan* p, hipStream_t st) {
    const bool dfmc = (p->variant == SKF_DFMC);
    if (dfmc && p->first_iter) zero_unknown_entries(p, st);
    p->first_iter = false;

    std::vector<int> all;
    // ---- phase A (second stream when available): Gram_i and K_i = pinv(Gram_i).  They depend
    // only on G, exactly like the relation contractions of phase B, so the two phases overlap.
    // The Gram products use the whole chip and stay on the main stream; the pseudo-inverses are
    // three single-workgroup kernels with a long serial chain: they go to the second stream and
    // run underneath the relation contractions.
    // (Round 1 / 2 A-B: with the Gram products on the second stream as well the contractions slow down by what those
    // kernels take -- profiles/r02_pipeline_ab.txt.)
    hipStream_t sa = st;
    for (size_t i = 0; i < p->types.size(); ++i) {
        gram(p, p->types[i], 1, st);
        all.push_back((int)i);
    }
    if (p->overlap) {
        SKF_HIP(hipEventRecord(p->ev_fork, st));
        SKF_HIP(hipStreamWaitEvent(p->aux, p->ev_fork, 0));
        sa = p->aux;
    }
    plan_pinv(p, all, sa);
    if (p->sw.debug_pinv) {
        // diagnostics: verdict of the Cholesky fast path and the diagonal range of every Gram matrix
        SKF_HIP(hipStreamSynchronize(sa));
        std::vector<int> ok(p->types.size());
        SKF_HIP(hipMemcpy(ok.data(), p->eigOk.ptr, ok.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < p->types.size(); ++i) {
            const TypeState& t = p->types[i];
            std::vector<double> gm((size_t)t.c * t.c);
            SKF_HIP(hipMemcpy(gm.data(), t.Gram.ptr, gm.size() * 8, hipMemcpyDeviceToHost));
            double lo = 1e300, hi = 0.0;
            for (int k = 0; k < t.c; ++k) {
                lo = gm[(size_t)k * t.c + k] < lo ? gm[(size_t)k * t.c + k] : lo;
                hi = gm[(size_t)k * t.c + k] > hi ? gm[(size_t)k * t.c + k] : hi;
            }
            fprintf(stderr, "[skf pinv] type %zu c=%d chol_ok=%d diag min %.3e max %.3e\n", i, t.c, ok[i], lo, hi);
        }
    }
    if (p->overlap) SKF_HIP(hipEventRecord(p->ev_join, p->aux));

    // ---- phase B (main stream): every product that streams a relation matrix, and W = G_i^T P
    for (RelState& r : p->rels) {
        TypeState& ti = p->types[r.row];
        TypeState& tj = p->types[r.col];
        // A masked DFMC relation is contracted twice per iteration: here, before its completion, only
        // W = G_i^T R G_j is needed (_dfmc.py:311-314), and the narrower factor does it -- with c_i < c_j as
        // W = (R^T G_i)^T G_j (config 5, user x movie: rank 128 instead of 256 through the 8 GB relation).
        const bool w_by_q = dfmc && r.masked && ti.c < tj.c;
        if (r.kn) {                 // known entries only: W from the stored residuals and c x c cross-Gram products
            known_w(p, r, st);
            continue;
        }
        if (r.absent) {
            SKF_HIP(hipMemsetAsync(r.W.ptr, 0, r.W.bytes, st));
        } else if (w_by_q) {
            contraction_Q(p, r, st);
            w_product(p, r, true, st);
        } else {
            contraction_P(p, r, st);
        }
        if (!(dfmc && r.masked)) contraction_Q(p, r, st);     // a masked relation is completed first
        if (!r.absent && !w_by_q) w_product(p, r, false, st);
    }
    if (p->overlap) SKF_HIP(hipStreamWaitEvent(st, p->ev_join, 0));
}

// Stage 2 (SKF_STAGE_BACKBONE): S = K_i W K_j; DFMC: completion, then P and Q of masked relations.
static void stage_backbone(skf_plan* p, hipStream_t st) {
    const bool dfmc = (p->variant == SKF_DFMC);
    const bool chain = small_chain(p);
    if (chain)
        for (size_t k0 = 0; k0 < p->rels.size(); k0 += CHAIN_MAXB)
            backbone_small_batch(p, k0, (int)std::min<size_t>(CHAIN_MAXB, p->rels.size() - k0), st);
    for (RelState& r : p->rels) {
        if (!chain) backbone_product(p, r, false, st);      // (rounded in stage_accumulate, with the B sums, in one launch)
        if (!(dfmc && r.masked)) continue;
        if (r.kn) {                 // completion, P and Q of _dfmc.py:319-325, 341-345 on the known entries
            known_operands(p, r, st, false);
            known_row_pass(p, r, st);
            known_col_pass(p, r, st);
            continue;
        }
        if (!r.absent) {
            // H = G_i[blk] S ; Rw[mask] = (H G_j^T)[mask] ; P = Rw G_j        (_dfmc.py:319-325)
            completion_operands(p, r, false, st);
            if (r.mask) complete_masked(p, r, st);
            contraction_P(p, r, st);
        }
        contraction_Q(p, r, st);
    }
}

// Stage 3 (SKF_STAGE_ACCUMULATE): the E / D sums of this plan's row blocks, column sides and constraints.
static void stage_accumulate(skf_plan* p, hipStream_t st) {
    const bool dfmc = (p->variant == SKF_DFMC);
    const int nan_upd = dfmc ? 0 : 1;       // _update_G_for_Rij (_dfmc.py:127-178) has no nan_to_num
    const bool fused = (p->engine == SKF_ENGINE_MFMA);
    const size_t nt = p->types.size();
    std::vector<char> touched(nt, 0);       // E/D of the type already written this iteration
    std::vector<int> sides_left(nt, 0);     // E/D side products still to come for the type
    for (RelState& r : p->rels) {
        if (!r.absent) sides_left[r.row] += 1;
        if (r.col_side) sides_left[r.col] += 1;
    }
    for (size_t i = 0; i < nt; ++i) {
        TypeState& t = p->types[i];
        // the fused update overwrites E/D on first touch -- of whole matrices only
        if (!fused || sides_left[i] == 0 || p->sliced) {
            SKF_HIP(hipMemsetAsync(t.E.ptr, 0, t.E.bytes, st));
            SKF_HIP(hipMemsetAsync(t.D.ptr, 0, t.D.bytes, st));
            touched[i] = 1;
        }
    }
    SKF_HIP(hipMemsetAsync((char*)p->ws_base + p->btot_off, 0, p->btot_bytes, st));
    // sum_r B_r^+- per type.  A plan with row blocks lists every relation and owns a share of the rows
    // of every type: it sums over all relations; otherwise over the plan's own relations.
    const bool chain = small_chain(p);
    for (RelState& r : p->rels) {
        if (chain) bterms_small(p, r, nan_upd, st);
        else bd_terms(p, r, nan_upd, nullptr, st);
    }
    // c x c operands of the fused side products in the master type: the f32 engines round S of every
    // relation with a side here and sum B+- of every type in ONE batched launch
    std::vector<const void*> Bn_m(nt), Bp_m(nt), S_m(p->rels.size());
    {
        const bool cast = !p->f64 && fused;
        CastBatch cb;
        int ne = 0, max_count = 1;
        auto add = [&](const Slot& src, const Slot& dst, int count) -> const void* {
            if (!cast) return src.ptr;
            if (ne >= CAST_MAXB) {                   // very large graphs: one launch per matrix
                hipLaunchKernelGGL((cast_kernel<float, double>), dim3(elem_grid(count)), dim3(256), 0, st, (float*)dst.ptr,
                                   (int64_t)count, (const double*)src.ptr, (int64_t)count, (int64_t)1, (int64_t)count);
                check_launch("cast");
                return dst.ptr;
            }
            cb.src[ne] = (const double*)src.ptr;
            cb.dst[ne] = (float*)dst.ptr;
            cb.count[ne] = count;
            if (count > max_count) max_count = count;
            ++ne;
            return dst.ptr;
        };
        for (size_t i = 0; i < nt; ++i) {
            TypeState& t = p->types[i];
            Bn_m[i] = add(t.Bn_tot, t.Bn32, t.c * t.c);
            Bp_m[i] = add(t.Bp_tot, t.Bp32, t.c * t.c);
        }
        for (size_t k = 0; k < p->rels.size(); ++k) {
            RelState& r = p->rels[k];
            S_m[k] = (!r.absent || r.col_side) ? add(r.S, r.S32, p->types[r.row].c * p->types[r.col].c) : r.S.ptr;
        }
        if (cast && ne > 0) {
            hipLaunchKernelGGL(cast_batched_kernel, dim3(elem_grid(max_count), ne), dim3(256), 0, st, cb);
            check_launch("cast_batched");
        }
    }
    // type-level term on rows [t0, t0 + tn): separately (row blocks / VALU engine), or inside the
    // last side product of the type (fused engine on whole matrices)
    auto type_term_of = [&](size_t i) {
        TypeState& t = p->types[i];
        if (t.tn <= 0) return;
        type_term(p, t, t.t0, t.tn, Bn_m[i], Bp_m[i], touched[i] != 0, fused, st);
        touched[i] = 1;
    };
    const bool fuse_type_term = fused && !p->sliced;
    for (size_t rk = 0; rk < p->rels.size(); ++rk) {
        RelState& r = p->rels[rk];
        if (!r.absent) {
            const bool last = fuse_type_term && --sides_left[r.row] == 0;
            if (r.kn) known_row_side(p, r, touched[r.row] != 0, st, false);
            else row_side(p, r, fused, S_m[rk], Bn_m[r.row], Bp_m[r.row], last, touched[r.row] != 0, nan_upd, st);
            touched[r.row] = 1;
            if (r.kn && last) type_term_of(r.row);
        }
        if (r.col_side) {
            const bool last = fuse_type_term && --sides_left[r.col] == 0;
            col_side(p, r, fused, 0, p->types[r.col].n, S_m[rk], Bn_m[r.col], Bp_m[r.col], last, touched[r.col] != 0, nan_upd, st);
            touched[r.col] = 1;
        }
    }
    if (!fuse_type_term)
        for (size_t i = 0; i < nt; ++i) type_term_of(i);     // E_i += G_i sum B- ; D_i += G_i sum B+
    theta_terms(p, st);
}

// E/D accumulation of one iteration: everything of the loop body except the final G update.
// With relation sharding every rank runs this on ITS relations / constraints, the E and D
// accumulators are then summed over the ranks (one all-reduce), and apply_update follows.
static void accumulate_fit(skf_plan* p, hipStream_t st) {
    stage_contract(p, st);
    stage_backbone(p, st);
    stage_accumulate(p, st);
}

// G_i <- G_i * sqrt(E_i / max(D_i, eps)) of every type (`done`: types the schedule has updated already); SKF_BF16: the
// update refreshes the bf16 copies of the factor in the same pass
static void apply_update(skf_plan* p, hipStream_t st, const std::vector<char>* done = nullptr) {
    for (TypeState& t : p->types)          // known-entries relations: the factors their stored residuals belong to
        if (t.keep_prev) SKF_HIP(hipMemcpyAsync(t.Gp.ptr, t.G.ptr, t.G.bytes, hipMemcpyDeviceToDevice, st));
    p->kn_first = false;
    for (size_t i = 0; i < p->types.size(); ++i)
        if (!(done && (*done)[i])) update_rows(p, p->types[i], 0, p->types[i].n, st);
}
