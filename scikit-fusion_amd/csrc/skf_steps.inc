// skf_steps.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): the steps of one iteration R_ij ~ G_i S_ij G_j^T, each stated ONCE.  A step fills its argument structs
// and launches on the stream it is given; it allocates nothing on the host and never synchronises (an iteration is captured
// into a hipGraph).  The three schedules -- staged (skf_stages.inc), relation pipeline (skf_schedule.inc), owned rows
// (skf_dist.inc) -- only order these steps: which stream, behind which event, in which order of the relations.  Where the
// schedules differ in HOW a step runs (where S is rounded, paired or unpaired B / D terms, split-K or not, whether the type
// term rides along) the difference is an argument here and a choice at the call site.
// ------------------------------------------------------------------------------------------
// every rank <= SMALLC: the c x c chains run in the one-workgroup kernels (SKF_NO_SMALL_CHAIN=1: off)
static bool small_chain(const skf_plan* p) {
    if (p->sw.no_small_chain) return false;
    for (const TypeState& t : p->types)
        if (t.c > SMALLC) return false;
    return true;
}

// May the c x c chains of the relations run on the second stream, underneath the contractions of the main one?
static bool chains_fit_second_stream(const skf_plan* p) {
    for (const ThetaState& th : p->thetas)
        if (!th.sparse) return false;            // (dense constraint products share the split-K scratch of the main stream)
    // above 512 (DFMC: 256) a c x c product on the second stream could ask for the main stream's split-K scratch;
    // every rank <= 64: launch-bound graphs, the one-workgroup chains on one stream are the faster path
    const int cmax = (p->variant == SKF_DFMC) ? 256 : 512;
    bool all_small = true;
    for (const TypeState& t : p->types) {
        if (t.c > cmax) return false;
        if (t.c > SMALLC) all_small = false;
    }
    return !all_small;
}

// W = G_i[blk]^T P over the rows of the block, or (by_q) W = Q^T G_j = (R^T G_i)^T G_j through the other object dimension
static void w_product(skf_plan* p, RelState& r, bool by_q, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    GemmArgs g = by_q ? gemm_args(r.Q.ptr, 1, ti.c, tj.G.ptr, tj.c, 1, r.W.ptr, tj.c, ti.c, tj.c, (int)tj.n, EPI_STORE, 0)
                      : gemm_args(rows_of(p, ti.G, ti, r.r0), 1, ti.c, r.P.ptr, tj.c, 1, r.W.ptr, tj.c, ti.c, tj.c, (int)r.nr,
                                  EPI_STORE, 0);
    wide_gemm(p, g, st);
}

// ---- the backbone S = K_i W K_j and the B / D terms of the relation, one-workgroup form (every rank <= SMALLC) ----------
// K_i, K_j, W / S, Gram_i, Gram_j and the products between them live in LDS
static size_t chain_lds_bytes(int ci, int cj) { return ((size_t)ci * ci + 2 * (size_t)ci * cj + (size_t)cj * cj) * 8; }
static void allow_chain_lds() {
    static DeviceOnce once_bb, once_bt;
    allow_dynamic_lds(once_bb, backbone_small_kernel, 4 * SMALLC * SMALLC * 8);
    allow_dynamic_lds(once_bt, bterms_small_kernel, 4 * SMALLC * SMALLC * 8);
}
// S of the relations [first_rel, first_rel + count), count <= CHAIN_MAXB: one workgroup each, one launch
static void backbone_small_batch(skf_plan* p, size_t first_rel, int count, hipStream_t st) {
    BackboneBatch bb;
    size_t smem = 0;
    for (int q = 0; q < count; ++q) {
        RelState& r = p->rels[first_rel + q];
        bb.Ki[q] = (const double*)p->types[r.row].K.ptr;
        bb.Kj[q] = (const double*)p->types[r.col].K.ptr;
        bb.W[q] = (const double*)r.W.ptr;
        bb.S[q] = (double*)r.S.ptr;
        bb.ci[q] = p->types[r.row].c;
        bb.cj[q] = p->types[r.col].c;
        const size_t need = chain_lds_bytes(bb.ci[q], bb.cj[q]);
        if (need > smem) smem = need;
    }
    allow_chain_lds();
    hipLaunchKernelGGL(backbone_small_kernel, dim3(count), dim3(256), smem, st, bb);
    check_launch("backbone_small");
}
// B = S Gram_j S^T and D = S^T Gram_i S, split by sign into the B sums of the two types
static void bterms_small(skf_plan* p, RelState& r, int nan_upd, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    BTermsArgs ba;
    ba.S = (const double*)r.S.ptr; ba.Gram_i = (const double*)ti.Gram.ptr; ba.Gram_j = (const double*)tj.Gram.ptr;
    ba.Bp_i = (double*)ti.Bp_tot.ptr; ba.Bn_i = (double*)ti.Bn_tot.ptr;
    ba.Bp_j = (double*)tj.Bp_tot.ptr; ba.Bn_j = (double*)tj.Bn_tot.ptr;
    ba.ci = ti.c; ba.cj = tj.c; ba.nan_to_num = nan_upd;
    allow_chain_lds();
    hipLaunchKernelGGL(bterms_small_kernel, dim3(1), dim3(256), chain_lds_bytes(ti.c, tj.c), st, ba);
    check_launch("bterms_small");
}

// ---- the same through the GEMM launches (any rank) ------------------------------------------------------------------------
// T1 = K_i W ; S = T1 K_j.  round_S_here (f32 engines): the f32 rounding of S leaves the same launch.  Returns the backbone
// in the master type as far as it exists behind this call: S32 once rounded, else S.
static const void* backbone_product(skf_plan* p, RelState& r, bool round_S_here, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    const int ci = ti.c, cj = tj.c;
    GemmArgs g = gemm_args(ti.K.ptr, ci, 1, r.W.ptr, cj, 1, r.T1.ptr, cj, ci, cj, ci, EPI_STORE, 0);       // T1 = K_i W
    small_gemm(p, g, st);
    g = gemm_args(r.T1.ptr, cj, 1, tj.K.ptr, cj, 1, r.S.ptr, cj, ci, cj, cj, EPI_STORE, 1);                // S = T1 K_j
    if (round_S_here) {
        g.epi = EPI_STORE_F32;
        g.C2 = r.S32.ptr;
        g.ldc2 = cj;
    }
    small_gemm(p, g, st);
    return round_S_here ? r.S32.ptr : r.S.ptr;
}
// the B / D terms of the relation into the B sums of its two types; U2: a second c_i x c_j buffer (the paired form of
// relation_small_terms: two products per launch), or none
static void bd_terms(skf_plan* p, RelState& r, int nan_upd, void* U2, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    relation_small_terms(p, r, nan_upd, EPI_SPLIT_ACC, ti.Bp_tot.ptr, ti.Bn_tot.ptr, tj.Bp_tot.ptr, tj.Bn_tot.ptr, true, true, st, U2);
}
// both, as the schedules that walk relation by relation issue them
static const void* backbone_general(skf_plan* p, RelState& r, int nan_upd, bool round_S_here, void* U2, hipStream_t st) {
    const void* Sm = backbone_product(p, r, round_S_here, st);
    bd_terms(p, r, nan_upd, U2, st);
    return Sm;
}
// f32 engines: S32 = the f32 rounding of S in a launch of its own (where it did not leave the S launch); returns S32
static const void* round_backbone(skf_plan* p, RelState& r, hipStream_t st) {
    const int ci = p->types[r.row].c, cj = p->types[r.col].c;
    hipLaunchKernelGGL((cast_kernel<float, double>), dim3(elem_grid((int64_t)ci * cj)), dim3(256), 0, st, (float*)r.S32.ptr,
                       (int64_t)cj, (const double*)r.S.ptr, (int64_t)cj, (int64_t)ci, (int64_t)cj);
    check_launch("cast");
    return r.S32.ptr;
}

// ---- DFMC: completion of the unknown entries of a masked relation, R[unknown] = (H G_j^T)[unknown], H = G_i[blk] S ---------
// SKF_BF16: the bf16 H and G_j of the tile kernels (r.H must be current); gj_from_rows: G_j from the bf16 rows the type
// keeps (an owned-rows plan whose other owners' f32 rows are not gathered) instead of the f32 masters
static void tile_operands(skf_plan* p, RelState& r, bool gj_from_rows, hipStream_t st) {
    TypeState& tj = p->types[r.col];
    launch_to_bf16<float>((uint16_t*)r.Hb.ptr, r.ldhb, (const float*)r.H.ptr, (int64_t)tj.c, r.nr, tj.c, false, st);
    if (gj_from_rows)
        launch_to_bf16<uint16_t>((uint16_t*)r.Gb.ptr, r.ldhb, (const uint16_t*)tj.Grow.ptr, tj.ldrow, tj.n, tj.c, false, st);
    else
        launch_to_bf16<float>((uint16_t*)r.Gb.ptr, r.ldhb, (const float*)tj.G.ptr, (int64_t)tj.c, tj.n, tj.c, false, st);
}
// H = G_i[blk] S (unsplit: one K slice, for the second stream), then the bf16 operands of the completion tiles
static void completion_operands(skf_plan* p, RelState& r, bool unsplit, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    GemmArgs g = gemm_args(rows_of(p, ti.G, ti, r.r0), ti.c, 1, r.S.ptr, tj.c, 1, r.H.ptr, tj.c, (int)r.nr, tj.c, ti.c, EPI_STORE, 0);
    if (unsplit) mixed_gemm_unsplit(p, g, st);
    else mixed_gemm(p, g, st);
    if (p->bf16 && r.mask) tile_operands(p, r, !tj.gather_master, st);
}

// SKF_BF16: one elementwise pass over the stored relation against its reconstruction H G_j^T (r.H = G_i S must
// be current): DFMC completion of the unknown entries, or the squared residual into p->sqpart (one f64 per tile)
enum { MODE_COMPLETE = 0, MODE_SQERR = 1 };
static void launch_tile_epilogue(skf_plan* p, RelState& r, int mode, hipStream_t st, bool operands = true) {
    TypeState& tj = p->types[r.col];
    const int nr = (int)r.nr, nj = (int)tj.n;
    if (operands) tile_operands(p, r, false, st);
    Bf16GemmArgs g;
    memset(&g, 0, sizeof g);
    // transposed product: tile rows = relation columns (A = bf16 G_j), tile columns = relation rows (Bt = bf16 H)
    g.A = (const uint16_t*)r.Gb.ptr; g.Bt = (const uint16_t*)r.Hb.ptr;
    g.lda = r.ldhb; g.ldb = r.ldhb;
    g.M = nj; g.N = nr; g.Kp = (int)r.ldhb; g.k_chunk = (int)r.ldhb;
    g.a_kstep = 64; g.b_kstep = 64;
    g.R = (uint16_t*)r.Rb.ptr; g.ldr = r.ldrb;
    if (r.binary) { g.Rbits = (const uint8_t*)r.Bb.ptr; g.ldrbits = r.ldbb; }
    g.mbits = (const uint8_t*)r.Mb.ptr; g.ldmb = r.ldmb;
    g.sq = (double*)p->sqpart.ptr;
    if (mode == MODE_COMPLETE && r.use_klist) {
        g.koff = (const uint32_t*)r.Koff.ptr;
        g.klist = (const uint32_t*)r.Klist.ptr;
    }
    if (mode == MODE_COMPLETE) {
        // 128 relation columns x 256 relation rows per workgroup, 256 threads, 68 KiB of LDS: two workgroups per CU, one
        // tile's write-out under the other's K loop (3.9 vs 4.7 ms at config 5).  The residual pass only reads the
        // relation and is faster on the 256 x 256 tile (4.7 vs 4.9 ms): it stays there.
        dim3 grid(cdiv(nr, 256), cdiv(nj, 128));
        const int smem = 256 * (128 + 8) * 2;
        static DeviceOnce once;
        allow_dynamic_lds(once, gemm_bf16_kernel<256, 0, EPI_T_COMPLETE>, smem);
        hipLaunchKernelGGL((gemm_bf16_kernel<256, 0, EPI_T_COMPLETE>), grid, dim3(256), smem, st, g);
        check_launch("tile_epilogue_bf16");
        return;
    }
    dim3 grid(cdiv(nr, 256), cdiv(nj, 256));
    const int smem = (3 * 256 + 2 * 256) * 8 * 16;
    static DeviceOnce once;
    allow_dynamic_lds(once, gemm_bf16_v2_kernel<256, 0, false, EPI_T_SQERR>, smem);
    hipLaunchKernelGGL((gemm_bf16_v2_kernel<256, 0, false, EPI_T_SQERR>), grid, dim3(512), smem, st, g);
    check_launch("tile_epilogue_bf16");
}

// Rw[mask] = (H G_j^T)[mask]  (_dfmc.py:319-325) behind completion_operands
static void complete_masked(skf_plan* p, RelState& r, hipStream_t st) {
    TypeState& tj = p->types[r.col];
    if (p->bf16) {
        // completed entries go to the one stored copy as bf16: bf16 operands on the matrix cores,
        // the write-out is the bound (gemm_bf16_kernel<.., EPI_T_COMPLETE>)
        launch_tile_epilogue(p, r, MODE_COMPLETE, st, false);
        return;
    }
    GemmArgs g = gemm_args(r.H.ptr, tj.c, 1, tj.G.ptr, 1, tj.c, r.Rw.ptr, r.ldr, (int)r.nr, (int)tj.n, tj.c, EPI_MASKED_STORE, 0);
    g.mask = (const uint8_t*)r.Mb.ptr;
    g.ldmask = r.ldmb;
    g.mask_bits = 1;
    plan_gemm(p, g, st);
}

// ---- the E / D sums of the factor update -----------------------------------------------------------------------------------
// Both side products come fused (MFMA engine: side_update_kernel; Sm = the backbone in the master type; `accumulate` false
// overwrites E / D; phase2 adds the type term G Bn / G Bp of type_term in the same launch, Bn / Bp in the master type) or
// unfused (one EPI_SPLIT_ACC product reading the f64 backbone itself: it always adds, into E / D the schedule has zeroed).
// row side, on the rows of the block: E_i (+)= (P S^T)+ ; D_i (+)= (P S^T)-          (_dfmf.py:254-258, 278-279)
static void row_side(skf_plan* p, RelState& r, bool fused, const void* Sm, const void* Bn, const void* Bp, bool phase2,
                     bool accumulate, int nan_upd, hipStream_t st) {
    TypeState& ti = p->types[r.row];
    const int ci = ti.c, cj = p->types[r.col].c;
    void* G = rows_of(p, ti.G, ti, r.r0);
    void* E = rows_of(p, ti.E, ti, r.r0);
    void* D = rows_of(p, ti.D, ti, r.r0);
    if (fused) {        // Sop(k, j) = S[j][k]
        side_update(p, r.P.ptr, cj, cj, Sm, 1, cj, ti, G, E, D, (int)r.nr, Bn, Bp, phase2, accumulate, nan_upd, st);
        return;
    }
    GemmArgs g = gemm_args(r.P.ptr, cj, 1, r.S.ptr, 1, cj, E, ci, (int)r.nr, ci, cj, EPI_SPLIT_ACC, nan_upd);
    g.C2 = D;
    mixed_gemm(p, g, st);
}
// column side, on the rows [j0, j0 + nj) of the column type: E_j (+)= (Q S)+ ; D_j (+)= (Q S)-      (_dfmf.py:266-270, 281-282)
static void col_side(skf_plan* p, RelState& r, bool fused, int64_t j0, int64_t nj, const void* Sm, const void* Bn,
                     const void* Bp, bool phase2, bool accumulate, int nan_upd, hipStream_t st) {
    TypeState& tj = p->types[r.col];
    const int ci = p->types[r.row].c, cj = tj.c;
    const void* Q = (const char*)r.Q.ptr + (size_t)j0 * ci * p->esz;
    void* G = rows_of(p, tj.G, tj, j0);
    void* E = rows_of(p, tj.E, tj, j0);
    void* D = rows_of(p, tj.D, tj, j0);
    if (fused) {
        side_update(p, Q, ci, ci, Sm, cj, 1, tj, G, E, D, (int)nj, Bn, Bp, phase2, accumulate, nan_upd, st);
        return;
    }
    GemmArgs g = gemm_args(Q, ci, 1, r.S.ptr, cj, 1, E, cj, (int)nj, cj, ci, EPI_SPLIT_ACC, nan_upd);
    g.C2 = D;
    mixed_gemm(p, g, st);
}

// f32 engines: the B sums of a type rounded to the master type (one launch); f64: the sums themselves
struct BSums { const void* Bn; const void* Bp; };
static BSums b_sums_master(skf_plan* p, TypeState& t, hipStream_t st) {
    if (p->f64) return {t.Bn_tot.ptr, t.Bp_tot.ptr};
    cast_b_sums(t, st);
    return {t.Bn32.ptr, t.Bp32.ptr};
}
// The G_i B^-+ terms of _dfmf.py:278-282 are linear in B: they are added once per type with the sums of B^+ / B^- over the
// relations (half the n x c x c work of adding them relation by relation).  On the rows [r0, r0 + n) of the type:
// E (+)= G sum B- ; D (+)= G sum B+.  Fused: Bn / Bp in the master type; unfused: the f64 sums, always added.
static void type_term(skf_plan* p, TypeState& t, int64_t r0, int64_t n, const void* Bn, const void* Bp, bool accumulate, bool fused,
                      hipStream_t st) {
    void* G = rows_of(p, t.G, t, r0);
    void* E = rows_of(p, t.E, t, r0);
    void* D = rows_of(p, t.D, t, r0);
    if (fused) {
        side_update(p, nullptr, 0, 0, nullptr, 0, 0, t, G, E, D, (int)n, Bn, Bp, true, accumulate, 0, st);
        return;
    }
    GemmArgs g = gemm_args(G, t.c, 1, Bn, t.c, 1, E, t.c, (int)n, t.c, t.c, EPI_ACC, 0);
    mixed_gemm(p, g, st);
    g = gemm_args(G, t.c, 1, Bp, t.c, 1, D, t.c, (int)n, t.c, t.c, EPI_ACC, 0);
    mixed_gemm(p, g, st);
}
// E = D = 0 on the rows [r0, r0 + n) of the type
static void zero_ed_rows(skf_plan* p, TypeState& t, int64_t r0, int64_t n, hipStream_t st) {
    SKF_HIP(hipMemsetAsync(rows_of(p, t.E, t, r0), 0, (size_t)n * t.c * p->esz, st));
    SKF_HIP(hipMemsetAsync(rows_of(p, t.D, t, r0), 0, (size_t)n * t.c * p->esz, st));
}

// G <- G * sqrt(E / max(D, eps)) on the rows [r0, r0 + n) of the type   (_dfmf.py:294-296); SKF_BF16: the bf16 copies of
// those rows (G^T and the rows of the list passes) leave the same pass
static void update_rows(skf_plan* p, TypeState& t, int64_t r0, int64_t n, hipStream_t st) {
    if (!p->bf16) {
        mult_update_rows(p, t, r0, n, st);
        return;
    }
    hipLaunchKernelGGL(mult_update_transpose_kernel, dim3((unsigned)cdiv(t.c, 32), (unsigned)cdiv(n, 32)), dim3(256), 0, st,
                       (float*)rows_of(p, t.G, t, r0), (const float*)rows_of(p, t.E, t, r0), (const float*)rows_of(p, t.D, t, r0),
                       n, (int64_t)t.c, (uint16_t*)t.GTb.ptr + r0, t.ldgt, (uint16_t*)t.Grow.ptr + r0 * t.ldrow, t.ldrow);
    check_launch("mult_update_transpose");
}
