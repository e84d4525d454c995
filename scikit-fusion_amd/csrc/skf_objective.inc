// skf_objective.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): the squared error of one relation under the current factors, |R - G_i S G_j^T|^2 over the local rows,
// one function per form of the relation (RelForm, skf_plan.inc); the entry point skf_relation_sqerr only picks one.
// Everything accumulates in the plan's error partials (sqpart, f64): slot 0 collects the c x c trace terms, an error pass
// over lists writes one partial per wave behind it (capacity: LayoutMax::want_partials, skf_create.inc).

// slot 0 (+)= scale * <S2, A_i S1 B_j>   (c_i x c_j, f64; U and T1 of the relation as scratch)
static void trace_term(skf_plan* p, RelState& r, const void* Ai, const void* S1, const void* Bj, const void* S2, double scale,
                       bool first, hipStream_t st) {
    const int ci = p->types[r.row].c, cj = p->types[r.col].c;
    GemmArgs h = gemm_args(Ai, ci, 1, S1, cj, 1, r.U.ptr, cj, ci, cj, ci, EPI_STORE, 0);          // U = A_i S1
    small_gemm(p, h, st);
    h = gemm_args(r.U.ptr, cj, 1, Bj, cj, 1, r.T1.ptr, cj, ci, cj, cj, EPI_STORE, 0);             // T1 = U B_j
    small_gemm(p, h, st);
    hipLaunchKernelGGL(dot_small_kernel, dim3(1), dim3(256), 0, st, (const double*)S2, (const double*)r.T1.ptr,
                       (int64_t)ci * cj, scale, (double*)p->sqpart.ptr, first ? 0 : 1);
    check_launch("dot_small");
}
// the ending of the list forms: an error pass has written `waves` partials behind slot 0 (capacity checked before it
// launched); out = slot 0 + all of them
static void list_total(skf_plan* p, int waves, double* out, hipStream_t st) {
    hipLaunchKernelGGL((sum_partials_kernel<double>), dim3(1), dim3(256), 0, st, (const double*)p->sqpart.ptr, waves + 1, out);
    check_launch("sum_partials");
}
static void gram_of(skf_plan* p, const void* A, const void* B, void* C, int c, int64_t n, hipStream_t st) {      // C = A^T B (c x c)
    GemmArgs h = gemm_args(A, 1, c, B, c, 1, C, c, c, c, (int)n, EPI_STORE, 0);
    wide_gemm(p, h, st);
}

// REL_FOLD_KNOWN: the known-entry objective: sum over the stored entries of (v - <G_t[o], T[i]>)^2, one pass, nothing else
static void sqerr_fold_known(skf_plan* p, RelState& r, double* out, hipStream_t st) {
    SKF_HIP(hipMemsetAsync(p->sqpart.ptr, 0, sizeof(double), st));
    list_total(p, fold_known_err_pass(p, r, st, 1), out, st);
}

// REL_FOLD: as for sqerr_stored below: tr(S^T Gram_i S Gram_j) + sum over the stored entries of (r - x)^2 - x^2, the lists
// compressed along the target: x = <H[o], G_p[idx]>, H = G_t S (row side) or G_t S^T (column side)
static void sqerr_fold(skf_plan* p, RelState& r, double* out, hipStream_t st) {
    TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    const int nj = (int)tj.n, ci = ti.c, cj = tj.c;
    gram_of(p, ti.G.ptr, ti.G.ptr, r.Xi.ptr, ci, ti.n, st);
    gram_of(p, tj.G.ptr, tj.G.ptr, r.Xj.ptr, cj, tj.n, st);
    trace_term(p, r, r.Xi.ptr, r.S.ptr, r.Xj.ptr, r.S.ptr, 1.0, true, st);
    GemmArgs h = r.row == p->target ? gemm_args(ti.G.ptr, ci, 1, r.S.ptr, cj, 1, r.H.ptr, cj, (int)ti.n, cj, ci, EPI_STORE, 0)
                                    : gemm_args(tj.G.ptr, cj, 1, r.S.ptr, 1, cj, r.H.ptr, ci, nj, ci, cj, EPI_STORE, 0);
    mixed_gemm(p, h, st);
    list_total(p, fold_err_pass(p, r, st, 1), out, st);
}

// REL_STORED: |R - X|^2 = |X|^2 - 2 <R, X> + |R|^2 with X = G_i S G_j^T and R zero off its stored entries:
//     |X|^2 = tr(S^T Gram_i S Gram_j)   (c x c, f64)
//     |R|^2 - 2 <R, X> = sum over the stored entries of (r - x)^2 - x^2 ,  x = <(G_i S)[row], G_j[col]>
// -- one pass over the row lists, never the n_i x n_j reconstruction (reference: _dfmf.py:306-316 on the dense form).
// (slot 0 of the partials collects the trace term, the pass writes behind it)
// (row ownership: the Gram of the LOCAL rows of G_i -- the trace term is linear in it, so the ranks' values sum to
// the relation's error -- and H of those rows)
static void sqerr_stored(skf_plan* p, RelState& r, double* out, hipStream_t st) {
    TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    const int ni = (int)r.nr, ci = ti.c, cj = tj.c;
    const void* Gi_b = rows_of(p, ti.G, ti, r.r0);
    gram_of(p, Gi_b, Gi_b, r.Xi.ptr, ci, r.nr, st);
    gram_of(p, tj.G.ptr, tj.G.ptr, r.Xj.ptr, cj, tj.n, st);
    trace_term(p, r, r.Xi.ptr, r.S.ptr, r.Xj.ptr, r.S.ptr, 1.0, true, st);
    GemmArgs h = gemm_args(Gi_b, ci, 1, r.S.ptr, cj, 1, r.H.ptr, cj, ni, cj, ci, EPI_STORE, 0);           // H = G_i S
    mixed_gemm(p, h, st);
    if (r.fill) fill_err_terms(p, r, st);                     // the rank-one terms into slot 0, beside the trace term
    list_total(p, sparse_pass(p, r, false, true, nullptr, st, 1), out, st);
}

// REL_KNOWN: the completed relation of _dfmc.py:385-386 is X_o + E (X_o = G_i,prev S_prev G_j,prev^T, E the stored
// residuals); with X_n = G_i S G_j^T of the current factors
//     |R_c - X_n|^2 = |X_o - X_n|^2 + sum over the known entries of (r - x_n)^2 - (x_o - x_n)^2 ,  x_o = r - e
// the first term from c x c Gram / cross-Gram products, the second from one pass over the column lists.
// (the partial slots [1, waves] belong to the pass below; slot 0 collects the trace terms)
static void sqerr_known(skf_plan* p, RelState& r, double* out, hipStream_t st) {
    TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    const int nj = (int)tj.n, ci = ti.c, cj = tj.c;
    const void* Gi_b = rows_of(p, ti.G, ti, r.r0);                   // the rows of the block (row ownership: the local ones)
    const void* Gp_b = ti.Gp.ptr ? rows_of(p, ti.Gp, ti, r.r0) : nullptr;
    gram_of(p, Gi_b, Gi_b, r.Xi.ptr, ci, r.nr, st);
    gram_of(p, tj.G.ptr, tj.G.ptr, r.Xj.ptr, cj, tj.n, st);
    trace_term(p, r, r.Xi.ptr, r.S.ptr, r.Xj.ptr, r.S.ptr, 1.0, true, st);
    if (!p->kn_first) {
        gram_of(p, Gp_b, Gi_b, r.Xi.ptr, ci, r.nr, st);                     // G_i,prev^T G_i
        gram_of(p, tj.G.ptr, tj.Gp.ptr, r.Xj.ptr, cj, tj.n, st);            // G_j^T G_j,prev
        trace_term(p, r, r.Xi.ptr, r.S.ptr, r.Xj.ptr, r.Sp.ptr, -2.0, false, st);
        gram_of(p, Gp_b, Gp_b, r.Xi.ptr, ci, r.nr, st);
        gram_of(p, tj.Gp.ptr, tj.Gp.ptr, r.Xj.ptr, cj, tj.n, st);
        trace_term(p, r, r.Xi.ptr, r.Sp.ptr, r.Xj.ptr, r.Sp.ptr, 1.0, false, st);
    }
    GemmArgs g2 = gemm_args(tj.G.ptr, cj, 1, r.S.ptr, 1, cj, r.Tm.ptr, ci, nj, ci, cj, EPI_STORE, 0);  // T = G_j S^T
    mixed_gemm(p, g2, st);
    if (p->bf16) launch_to_bf16<float>((uint16_t*)r.FiB.ptr, r.kn_ldf, (const float*)r.Tm.ptr, (int64_t)ci, tj.n, ci, false, st);
    list_total(p, known_pass(p, r, true, SRP_ERR, st, 1), out, st);
}

// REL_DENSE: H = G_i S, then the residual against the stored matrix, tile by tile (reference: _dfmf.py:306-316)
static void sqerr_dense(skf_plan* p, RelState& r, double* out, hipStream_t st) {
    TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    const int ni = (int)r.nr, nj = (int)tj.n, ci = ti.c, cj = tj.c;        // the local rows
    GemmArgs g = gemm_args(rows_of(p, ti.G, ti, r.r0), ci, 1, r.S.ptr, cj, 1, r.H.ptr, cj, ni, cj, ci, EPI_STORE, 0);
    mixed_gemm(p, g, st);
    if (p->bf16) {
        // one pass over the stored bf16 relation: bf16 H and G_j on the matrix cores, f32 residual
        launch_tile_epilogue(p, r, MODE_SQERR, st);
        list_total(p, cdiv(ni, 256) * cdiv(nj, 256) - 1, out, st);       // (one f64 partial per tile, the first in slot 0)
        return;
    }
    g = gemm_args(r.H.ptr, cj, 1, tj.G.ptr, 1, cj, (void*)r.R, r.ldr, ni, nj, cj, EPI_SQDIFF, 0);
    g.C2 = p->sqpart.ptr;
    // one partial per workgroup of the tile run_gemm picks for THIS product (an all-f64 product of a small
    // relation with 64 <= c_j <= 1024 runs on the deep 32 x 32 tile)
    const TileCfg t = gemm_tile(GemmTypes{p->mt, p->mt, p->mt}, p->engine, g, p->f64, false);
    const int blocks = cdiv(ni, t.bm) * cdiv(nj, t.bn);
    if ((size_t)blocks > p->sq_elems) SKF_FAIL(SKF_E_STATE, "residual partials: %d tiles > %zu slots", blocks, p->sq_elems);
    plan_gemm(p, g, st);
    if (p->f64)
        hipLaunchKernelGGL((sum_partials_kernel<double>), dim3(1), dim3(256), 0, st, (const double*)p->sqpart.ptr,
                           blocks, out);
    else
        hipLaunchKernelGGL((sum_partials_kernel<float>), dim3(1), dim3(256), 0, st, (const float*)p->sqpart.ptr,
                           blocks, out);
    check_launch("sum_partials");
}
