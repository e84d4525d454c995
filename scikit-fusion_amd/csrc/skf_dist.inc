// skf_dist.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): collectives behind the boundary (RCCL by dlopen, callbacks, the null communicator) and the sharded
// iterations: skf_iterate_dist, which cuts the staged schedule between its collectives, and the OWNED-ROWS schedule, which
// orders the steps of skf_steps.inc over three streams with the exchanges between them.
// ------------------------------------------------------------------------------------------
// Collectives behind the boundary (include/skfusion_hip.h, skf_comm_*): RCCL bound at run time with dlopen -- no
// torch, no link-time dependency -- or caller-supplied callbacks (CPU tests over gloo, other transports).
// ------------------------------------------------------------------------------------------
struct NcclUniqueId { char internal[128]; };
typedef int (*nccl_get_unique_id_t)(NcclUniqueId*);
typedef int (*nccl_comm_init_rank_t)(void**, int, NcclUniqueId, int);
typedef int (*nccl_comm_destroy_t)(void*);
typedef int (*nccl_all_reduce_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_reduce_scatter_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_all_gather_t)(const void*, void*, size_t, int, void*, hipStream_t);
typedef const char* (*nccl_get_error_string_t)(int);
typedef int (*nccl_comm_count_t)(const void*, int*);
struct Rccl {
    nccl_comm_count_t comm_count = nullptr;          // optional (skf_comm_info)
    nccl_comm_count_t comm_user_rank = nullptr;
    void* handle = nullptr;
    nccl_get_unique_id_t get_unique_id = nullptr;
    nccl_comm_init_rank_t comm_init_rank = nullptr;
    nccl_comm_destroy_t comm_destroy = nullptr;
    nccl_all_reduce_t all_reduce = nullptr;
    nccl_reduce_scatter_t reduce_scatter = nullptr;
    nccl_all_gather_t all_gather = nullptr;
    nccl_get_error_string_t error_string = nullptr;
};
static Rccl g_rccl;
static std::once_flag g_rccl_once;

// librccl of the process if one is loaded already (PyTorch-ROCm bundles its own), else SKF_RCCL_PATH / the loader path / ROCm
static const Rccl& rccl() {
    std::call_once(g_rccl_once, [] {
        const char* names[] = {env_str("SKF_RCCL_PATH"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
        void* h = nullptr;
        for (const char* nm : names)
            if (nm && !h) h = dlopen(nm, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
        for (const char* nm : names)
            if (nm && !h) h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        g_rccl.handle = h;
        g_rccl.get_unique_id = (nccl_get_unique_id_t)dlsym(h, "ncclGetUniqueId");
        g_rccl.comm_init_rank = (nccl_comm_init_rank_t)dlsym(h, "ncclCommInitRank");
        g_rccl.comm_destroy = (nccl_comm_destroy_t)dlsym(h, "ncclCommDestroy");
        g_rccl.all_reduce = (nccl_all_reduce_t)dlsym(h, "ncclAllReduce");
        g_rccl.reduce_scatter = (nccl_reduce_scatter_t)dlsym(h, "ncclReduceScatter");
        g_rccl.all_gather = (nccl_all_gather_t)dlsym(h, "ncclAllGather");
        g_rccl.error_string = (nccl_get_error_string_t)dlsym(h, "ncclGetErrorString");
        g_rccl.comm_count = (nccl_comm_count_t)dlsym(h, "ncclCommCount");
        g_rccl.comm_user_rank = (nccl_comm_count_t)dlsym(h, "ncclCommUserRank");
    });
    if (!g_rccl.handle || !g_rccl.get_unique_id || !g_rccl.comm_init_rank || !g_rccl.comm_destroy || !g_rccl.all_reduce ||
        !g_rccl.reduce_scatter || !g_rccl.all_gather)
        SKF_FAIL(SKF_E_STATE, "librccl.so could not be loaded (set SKF_RCCL_PATH, or use skf_comm_create_callback)");
    return g_rccl;
}

}  // namespace skf

struct skf_comm {
    int rank = 0, world = 1;
    void* nccl = nullptr;                  // ncclComm_t, or
    skf_collective_fn fn = nullptr;        // caller-supplied collectives
    void* user = nullptr;
    bool null_comm = false;                // collectives skipped (skf_comm_create_null)
};

namespace skf {

enum { COLL_ALL_REDUCE = 0, COLL_REDUCE_SCATTER = 1, COLL_ALL_GATHER = 2 };

// op over `count` elements per rank (COLL_ALL_REDUCE: the whole buffer; the other two: chunk `rank` of world * count), in place
static void collective(skf_comm* c, int op, void* buf, size_t count, int dtype, hipStream_t st) {
    if (!c) SKF_FAIL(SKF_E_STATE, "no communicator attached to the plan (skf_plan_set_comm)");
    if (count == 0) return;
    if (c->fn) {
        const int rc = c->fn(c->user, op, buf, count, dtype, (void*)st);
        if (rc != 0) SKF_FAIL(SKF_E_HIP, "collective callback failed (op %d, status %d)", op, rc);
        return;
    }
    if (c->null_comm) {
        // timing runs of ONE rank of a sharded fit (skf_comm_create_null): nothing is exchanged; a sum over the ranks is stood
        // in for by `world` times this rank's partial, so that the Gram matrices, backbones and updates the timed launches see
        // stay in the range of a real run (a Gram matrix of 1/8 of the rows sends the factors off scale, and the
        // pseudo-inverses then take their slow fallbacks); gathered rows of other ranks keep their old values
        if (op == COLL_ALL_GATHER || c->world == 1 || dtype == SKF_BF16) return;
        const size_t es = dtype == SKF_F64 ? 8 : 4;
        char* at = (char*)buf + (op == COLL_REDUCE_SCATTER ? (size_t)c->rank * count * es : 0);
        if (dtype == SKF_F64)
            hipLaunchKernelGGL((scale_kernel<double>), dim3(elem_grid((int64_t)count)), dim3(256), 0, st, (double*)at, (int64_t)count, (double)c->world);
        else
            hipLaunchKernelGGL((scale_kernel<float>), dim3(elem_grid((int64_t)count)), dim3(256), 0, st, (float*)at, (int64_t)count, (float)c->world);
        check_launch("scale (null communicator)");
        return;
    }
    if (c->world == 1 && !c->nccl) return;          // a single rank without a transport: nothing to exchange
    const Rccl& r = rccl();
    const int nt = dtype == SKF_F64 ? 8 /* ncclFloat64 */ : 7 /* ncclFloat32 */;
    const size_t es = dtype == SKF_F64 ? 8 : dtype == SKF_BF16 ? 2 : 4;
    char* mine = (char*)buf + (size_t)c->rank * count * es;
    int rc = 0;
    if (dtype == SKF_BF16 && op != COLL_ALL_GATHER) SKF_FAIL(SKF_E_INVALID, "bf16 collectives: all-gather only");
    if (op == COLL_ALL_REDUCE) rc = r.all_reduce(buf, buf, count, nt, 0 /* ncclSum */, c->nccl, st);
    else if (op == COLL_REDUCE_SCATTER) rc = r.reduce_scatter(buf, mine, count, nt, 0, c->nccl, st);
    else if (dtype == SKF_BF16) rc = r.all_gather(mine, buf, count * 2, 1 /* ncclUint8: the bytes of the bf16 rows */, c->nccl, st);
    else rc = r.all_gather(mine, buf, count, nt, c->nccl, st);
    if (rc != 0) SKF_FAIL(SKF_E_HIP, "RCCL collective %d failed: %s", op, r.error_string ? r.error_string(rc) : "?");
}

// elements per rank when `total` elements are cut into `world` equal ranges (multiples of 64; the region's pad takes the rest)
static size_t flat_chunk(size_t total, int world) { return ((total + world - 1) / world + 63) / 64 * 64; }

// One iteration with the exchanges inside: plans without row blocks run accumulate -> exchange -> update, plans with row
// blocks the four stages.  E / D: reduce-scatter (every rank ends with the sums of ITS element range), update of that
// range of G, all-gather of G -- (2 + 1) * (world - 1) / world of the factor bytes per rank instead of the
// 2 * 2 * (world - 1) / world of an all-reduce of both accumulators.
static void exchange_and_update(skf_plan* p, hipStream_t st) {
    skf_comm* c = p->comm;
    const size_t total = p->flat_bytes / p->esz;
    const size_t chunk = flat_chunk(total, c->world);
    if (chunk * c->world * p->esz > p->flat_bytes + 64 * 1024) SKF_FAIL(SKF_E_STATE, "exchange ranges exceed the region pad (world %d)", c->world);
    char* base = (char*)p->ws_base;
    void* E = base + p->flat_e_off;
    void* D = base + p->flat_d_off;
    void* G = base + p->flat_g_off;
    collective(c, COLL_REDUCE_SCATTER, E, chunk, p->mt, st);
    collective(c, COLL_REDUCE_SCATTER, D, chunk, p->mt, st);
    for (TypeState& t : p->types)          // known-entries relations: the factors their stored residuals belong to
        if (t.keep_prev) SKF_HIP(hipMemcpyAsync(t.Gp.ptr, t.G.ptr, t.G.bytes, hipMemcpyDeviceToDevice, st));
    p->kn_first = false;
    const size_t lo = (size_t)c->rank * chunk;
    if (p->f64)
        hipLaunchKernelGGL((mult_update_kernel<double>), dim3(elem_grid((int64_t)chunk)), dim3(256), 0, st, (double*)G + lo,
                           (const double*)E + lo, (const double*)D + lo, (int64_t)chunk, 1, (int64_t)1, (int64_t)1);
    else
        hipLaunchKernelGGL((mult_update_kernel<float>), dim3(elem_grid((int64_t)chunk)), dim3(256), 0, st, (float*)G + lo,
                           (const float*)E + lo, (const float*)D + lo, (int64_t)chunk, 1, (int64_t)1, (int64_t)1);
    check_launch("mult_update(range)");
    collective(c, COLL_ALL_GATHER, G, chunk, p->mt, st);
    for (TypeState& t : p->types) refresh_gt(p, t, st);
}

static void iterate_dist(skf_plan* p, hipStream_t st) {
    skf_comm* c = p->comm;
    char* base = (char*)p->ws_base;
    if (!p->sliced) {
        accumulate_fit(p, st);
    } else {
        stage_contract(p, st);
        collective(c, COLL_ALL_REDUCE, base + p->xw_off, p->xw_bytes / 8, SKF_F64, st);
        collective(c, COLL_ALL_REDUCE, base + p->xq_off, p->xq_bytes / p->esz, p->mt, st);
        stage_backbone(p, st);
        collective(c, COLL_ALL_REDUCE, base + p->xqm_off, p->xqm_bytes / p->esz, p->mt, st);
        stage_accumulate(p, st);
    }
    exchange_and_update(p, st);
}

// bytes one rank SENDS per iteration of skf_iterate_dist on a ring (reduce-scatter / all-gather: (world-1)/world of the
// buffer, all-reduce: twice that)
static size_t exchange_bytes(const skf_plan* p, int world) {
    if (world <= 1) return 0;
    const double f = (double)(world - 1) / world;
    if (p->owned) {
        // reduce-scatter of every relation's partial Q, all-gather of every type's updated rows (master type, or the bf16
        // operand rows), all-reduce of the c x c Gram and W partials
        double b = 0.0;
        for (const RelState& r : p->rels) b += f * (double)p->types[r.col].n_alloc * p->types[r.row].c * (double)p->esz;
        for (const TypeState& t : p->types)
            b += f * (double)t.n_alloc * (t.gather_master ? (double)t.c * (double)p->esz : (double)t.ldrow * 2.0);
        b += 2.0 * f * (double)p->xg_bytes;                 // (the Gram range goes out as a whole, slot padding included)
        for (const RelState& r : p->rels) b += 2.0 * f * 8.0 * (double)p->types[r.row].c * p->types[r.col].c;
        return (size_t)(b + 0.5);
    }
    double b = 3.0 * f * (double)(flat_chunk(p->flat_bytes / p->esz, world) * world * p->esz);
    if (p->sliced) b += 2.0 * f * (double)(p->xw_bytes + p->xq_bytes + p->xqm_bytes);
    return (size_t)b;
}

// ------------------------------------------------------------------------------------------
// SKF_OPT_OWNED_ROWS: one iteration of a fit whose row blocks follow the OWNERSHIP of the factor rows (every rank holds the
// rows [t0, t0 + tn) of every type: of its factor, of E / D, of every relation with that row type).  Replaces the
// reference's per-block tasks (_dfmf.py:69-73, _dfmc.py:341-345).  What crosses ranks:
//     Gram_t = sum over ranks of G_t[own]^T G_t[own]            all-reduce, c x c f64, all types at once
//     W_r    = sum over ranks of G_i[own]^T (R_blk G_j)         all-reduce, c_i x c_j f64, per relation
//     Q_r    = sum over ranks of R_blk^T G_i[own]               REDUCE-SCATTER to the owners of type j (raw: the +- split of
//                                                               _dfmf.py:268-270 is not linear), per relation
//     G_t                                                       ALL-GATHER of the updated owned rows, per type (SKF_BF16: of
//                                                               their bf16 operand copy unless a constraint reads the f32 rows)
// Row sides (P S^T)+-, type terms G_i sum B-+, constraint rows and the update act on owned rows: no exchange of E / D.
// Three streams when the graph allows (ranks in 65 .. 512, sparse constraints only -- the conditions under which the c x c
// chains need no split-K scratch): main = Gram, contractions, W; second = pseudo-inverses, backbones, side products,
// updates; `cs` = the exchanges.  A relation's exchanges run under the next relation's contractions, a type is updated and
// gathered as soon as its last relation's sides are in.  Otherwise everything is issued in the same order on one stream.
// ------------------------------------------------------------------------------------------
static bool owned_can_overlap(const skf_plan* p) {
    if (!p->overlap || p->engine != SKF_ENGINE_MFMA) return false;
    // every rank <= 64: launch-bound graphs, one stream.  Mixed ranks (config 5: 16 ... 256) do overlap: the replicated
    // pseudo-inverses (0.65 ms at order 256) then run beside the list passes instead of in front of them.
    return chains_fit_second_stream(p);
}

static void iterate_owned(skf_plan* p, hipStream_t st) {
    skf_comm* c = p->comm;
    const size_t nt = p->types.size(), nr = p->rels.size();
    const bool dfmc = (p->variant == SKF_DFMC);
    const int nan_upd = dfmc ? 0 : 1;
    const bool fused = (p->engine == SKF_ENGINE_MFMA);
    const bool multi = owned_can_overlap(p);
    hipStream_t ax = multi ? p->aux : st;
    hipStream_t cs = (multi && p->cs) ? p->cs : st;
    char* base = (char*)p->ws_base;
    if (dfmc && p->first_iter) zero_unknown_entries(p, st);
    p->first_iter = false;
    // events: [0] Gram partials, [1] Gram sums; per relation: W partial, W sum, Q partial, Q scattered, backbone (+ completion
    // operands), P after the completion; per type: rows updated, rows gathered, operand copies refreshed
    const size_t n_ev = 2 + 6 * nr + 3 * nt;
    while (p->ev_own.size() < n_ev) {
        hipEvent_t e;
        SKF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        p->ev_own.push_back(e);
    }
    enum { R_W = 0, R_WX = 1, R_Q = 2, R_QX = 3, R_S = 4, R_P2 = 5, T_UPD = 0, T_G = 1, T_GT = 2 };
    auto ev_r = [&](size_t k, int what) { return p->ev_own[2 + 6 * k + what]; };
    auto ev_t = [&](size_t i, int what) { return p->ev_own[2 + 6 * nr + 3 * i + what]; };
    auto rec = [&](hipEvent_t e, hipStream_t s) { SKF_HIP(hipEventRecord(e, s)); };
    auto wait = [&](hipStream_t s, hipEvent_t e) { SKF_HIP(hipStreamWaitEvent(s, e, 0)); };
    auto own = [&](const Slot& s, const TypeState& t) { return rows_of(p, s, t, t.t0); };

    // ---- Gram partials over the owned rows (main stream, at the head: the chain Gram -> sum -> pseudo-inverses (~1.2 ms at
    // rank 256, one workgroup per type) -> backbones -> side products IS the critical path of a rank, the contractions run
    // beside it), their sum (exchange stream), the pseudo-inverses (second stream).
    // (Measured, rank 3 of 8 at config 3: with the partials on the second stream underneath the first contraction their
    // split-K reduce crawled for 0.26 ms, the pseudo-inverses started 0.33 ms later and the iteration took as long as
    // before -- 2.55 ms; profiles/r04_owned_rank_timeline.txt.)
    std::vector<int> all;
    hipStream_t sg = st;
    const bool gram_aux = false;
    if (gram_aux) {
        rec(p->ev_fork, st);                       // (factors set / updated on the caller's stream before this call)
        wait(ax, p->ev_fork);
    }
    std::vector<GemmArgs> shares;              // the Gram shares of the owned rows: one grouped launch (gram_group_try), or one by one
    for (size_t i = 0; i < nt; ++i) {
        TypeState& t = p->types[i];
        all.push_back((int)i);
        if (t.tn <= 0) {
            SKF_HIP(hipMemsetAsync(t.Gram.ptr, 0, t.Gram.bytes, sg));
            continue;
        }
        GemmArgs g = gemm_args(own(t.G, t), 1, t.c, own(t.G, t), t.c, 1, t.Gram.ptr, t.c, t.c, t.c, (int)t.tn, EPI_STORE, 1);
        g.sym = p->sw.gram_sym;
        shares.push_back(g);
    }
    {
        void* part = gram_aux ? p->part_aux.ptr : p->part.ptr;
        const size_t bytes = gram_aux ? p->part_aux_bytes : p->part_bytes;
        if (!gram_group_try(p, shares.data(), (int)shares.size(), part, bytes, sg))
            for (const GemmArgs& g : shares) kind_gemm(p, kind_gram(p), g, sg, gram_aux);
    }
    rec(p->ev_own[0], sg);
    wait(cs, p->ev_own[0]);
    collective(c, COLL_ALL_REDUCE, base + p->xg_off, p->xg_bytes / 8, SKF_F64, cs);
    rec(p->ev_own[1], cs);
    wait(ax, p->ev_own[1]);
    plan_pinv(p, all, ax);
    SKF_HIP(hipMemsetAsync(base + p->btot_off, 0, p->btot_bytes, ax));

    std::vector<char> touched(nt, 0);          // E / D of the type's owned rows already written this iteration
    std::vector<int> sides_left(nt, 0);        // side products of the type still to come
    for (const RelState& r : p->rels) {
        sides_left[r.row] += 1;
        sides_left[r.col] += 1;
    }
    std::vector<const void*> Sm(nr, nullptr);  // the backbone in the master type
    std::vector<char> finished(nt, 0);
    const bool chain = small_chain(p);

    // the type is complete: type term, constraint rows, update of the owned rows (second stream), gather (exchange stream)
    auto finish_type = [&](size_t i) {
        TypeState& t = p->types[i];
        finished[i] = 1;
        // known-entries relations: the factor their stored residuals belong to (all rows: every one is current here)
        if (t.keep_prev) SKF_HIP(hipMemcpyAsync(t.Gp.ptr, t.G.ptr, (size_t)t.n * t.c * p->esz, hipMemcpyDeviceToDevice, ax));
        if (t.tn > 0) {
            if (!touched[i]) {
                zero_ed_rows(p, t, t.t0, t.tn, ax);
                touched[i] = 1;
            }
            // (its own launch on the owned rows, the B sums rounded here for the fused form)
            const BSums b = fused ? b_sums_master(p, t, ax) : BSums{t.Bn_tot.ptr, t.Bp_tot.ptr};
            type_term(p, t, t.t0, t.tn, b.Bn, b.Bp, true, fused, ax);
            theta_terms_rows(p, (int)i, true, ax);
            // rank-emulation runs (skf_comm_create_null): the factors stay as they were set -- with nothing exchanged the
            // updated rows drift away from the rows of the ranks that do not exist, the Gram matrices go singular and the
            // timed pseudo-inverses take their slow fallbacks (measured: 4-15 ms per iteration); the update launch
            // itself (~10 us per type) is what the measurement then leaves out
            if (!c->null_comm) update_rows(p, t, t.t0, t.tn, ax);
        }
        rec(ev_t(i, T_UPD), ax);
        wait(cs, ev_t(i, T_UPD));
        if (t.gather_master) collective(c, COLL_ALL_GATHER, t.G.ptr, (size_t)t.chunk * t.c, p->mt, cs);
        else collective(c, COLL_ALL_GATHER, t.Grow.ptr, (size_t)t.chunk * t.ldrow, SKF_BF16, cs);
        rec(ev_t(i, T_G), cs);
        if (p->bf16) {      // the operand copies of ALL rows from what was gathered
            wait(ax, ev_t(i, T_G));
            if (t.gather_master) refresh_gt(p, t, ax);
            else launch_to_bf16<uint16_t>((uint16_t*)t.GTb.ptr, t.ldgt, (const uint16_t*)t.Grow.ptr, t.ldrow, t.n, (int64_t)t.c, true, ax);
            rec(ev_t(i, T_GT), ax);
        }
    };
    auto side_done = [&](int type) {
        if (--sides_left[type] == 0) finish_type((size_t)type);
    };
    // W partial of relation k from its P (main stream), then its sum (exchange stream)
    auto w_partial = [&](size_t k) {
        RelState& r = p->rels[k];
        TypeState& ti = p->types[r.row];
        TypeState& tj = p->types[r.col];
        if (r.absent) {
            SKF_HIP(hipMemsetAsync(r.W.ptr, 0, r.W.bytes, st));
        } else if (r.kn) {                  // lists of known entries: the block's share of W from its stored residuals (skf_known.h)
            known_w(p, r, st);
        } else {
            w_product(p, r, false, st);
        }
        rec(ev_r(k, R_W), st);
        wait(cs, ev_r(k, R_W));
        collective(c, COLL_ALL_REDUCE, r.W.ptr, (size_t)ti.c * tj.c, SKF_F64, cs);
        rec(ev_r(k, R_WX), cs);
    };
    // partial Q of relation k (main stream), then the rows of its sum this rank owns (exchange stream)
    auto q_partial = [&](size_t k) {
        RelState& r = p->rels[k];
        TypeState& ti = p->types[r.row];
        TypeState& tj = p->types[r.col];
        if (r.absent) SKF_HIP(hipMemsetAsync(r.Q.ptr, 0, (size_t)tj.n * ti.c * p->esz, st));
        else if (r.kn) known_pass(p, r, true, SRP_RESIDUAL, st);       // E^T G_i of the block's rows (the dense part of Q follows
        else contraction_Q(p, r, st);                                  //  the scatter, on the owned rows of the column type)
        rec(ev_r(k, R_Q), st);
        wait(cs, ev_r(k, R_Q));
        collective(c, COLL_REDUCE_SCATTER, r.Q.ptr, (size_t)tj.chunk * ti.c, p->mt, cs);
        rec(ev_r(k, R_QX), cs);
    };
    // second stream, behind the sum of W: S = K_i W K_j, its B / D terms, the rounding of S
    auto backbone_chain = [&](size_t k) {
        RelState& r = p->rels[k];
        wait(ax, ev_r(k, R_WX));
        // f32 engines, fused side products: the rounding of S leaves the S launch (the chain kernels have no such form)
        const bool s32_here = !chain && !p->f64 && fused && !p->sw.no_pairs;
        if (chain) {
            backbone_small_batch(p, k, 1, ax);
            bterms_small(p, r, nan_upd, ax);
            Sm[k] = r.S.ptr;
        } else {
            Sm[k] = backbone_general(p, r, nan_upd, s32_here, r.T1.ptr, ax);       // (paired: T1 is free once S is there)
        }
        if (!p->f64 && fused && !s32_here) Sm[k] = round_backbone(p, r, ax);
    };
    // second stream: row side on the local rows behind `ev_p`, column side on the owned rows of the column type behind the
    // scattered Q; E / D of the owned rows are overwritten (fused) or zeroed (unfused) on first touch
    auto side_products = [&](size_t k, hipEvent_t ev_p) {
        RelState& r = p->rels[k];
        TypeState& ti = p->types[r.row];
        TypeState& tj = p->types[r.col];
        const int ci = ti.c, cj = tj.c;
        wait(ax, ev_p);
        if (!r.absent && r.kn) {            // the row-side product P S^T = G_i (S Gram_j S^T) + E T was formed by the row pass
            known_row_split(p, r, touched[r.row] != 0, ax);
            touched[r.row] = 1;
        } else if (!r.absent) {
            if (!fused && !touched[r.row]) zero_ed_rows(p, ti, ti.t0, ti.tn, ax);
            row_side(p, r, fused, Sm[k], nullptr, nullptr, false, touched[r.row] != 0, nan_upd, ax);
            touched[r.row] = 1;
        }
        side_done(r.row);
        wait(ax, ev_r(k, R_QX));
        if (r.kn) {                         // Q = G_j (S^T Gram_i) + E^T G_i: the dense part on the owned rows, then S_prev <- S
            known_col_dense(p, r, tj.t0, tj.tn, ax, multi);
            if (!r.absent) copy2d(r.Sp.ptr, cj, r.S.ptr, cj, ci, cj, 8, ax);
        }
        if (tj.tn > 0) {
            if (!fused && !touched[r.col]) zero_ed_rows(p, tj, tj.t0, tj.tn, ax);
            col_side(p, r, fused, tj.t0, tj.tn, Sm[k], nullptr, nullptr, false, touched[r.col] != 0, nan_upd, ax);
            touched[r.col] = 1;
        }
        side_done(r.col);
    };

    // The launches go out stream by stream, not relation by relation: every contraction of the main stream is enqueued BEFORE
    // the chains of the second stream, whose first packets wait for the pseudo-inverses (~1.2 ms at rank 256).  Streams
    // share hardware queues, and a queue hands out its packets in order: issued relation by relation, the third relation's
    // contractions sat behind the first relation's waiting chain for 0.5 ms (rocprof timeline of rank 3 of 8, config 3).
    // ---- main stream (+ exchanges): masked relations (DFMC) before their completion: P, W (_dfmc.py:311-314) ...
    for (size_t k = 0; k < nr; ++k) {
        RelState& r = p->rels[k];
        if (!(dfmc && r.masked)) continue;
        if (!r.absent && !r.kn) contraction_P(p, r, st);
        w_partial(k);
    }
    // ... and the unmasked relations: P, W, Q
    for (size_t k = 0; k < nr; ++k) {
        RelState& r = p->rels[k];
        if (dfmc && r.masked) continue;
        if (!r.absent) contraction_P(p, r, st);
        w_partial(k);
        q_partial(k);
    }
    // ---- second stream: backbone, H = G_i[own] S and the completion operands of the masked relations ...
    for (size_t k = 0; k < nr; ++k) {
        RelState& r = p->rels[k];
        if (!(dfmc && r.masked)) continue;
        TypeState& ti = p->types[r.row];
        TypeState& tj = p->types[r.col];
        backbone_chain(k);
        if (r.kn) {                         // gathered vectors T = G_j S^T and the c x c operands of the dense parts
            if (!r.absent) {
                known_operands(p, r, ax, multi);
            } else {                        // (no rows of the relation here: only U2 = S^T Gram_i for this process's rows of Q)
                GemmArgs g = gemm_args(r.S.ptr, 1, tj.c, ti.Gram.ptr, ti.c, 1, r.U2.ptr, ti.c, tj.c, ti.c, ti.c, EPI_STORE, 0);
                small_gemm(p, g, ax);
            }
        } else if (!r.absent) {         // (bf16 operands of the completion tiles: G_j from what this rank holds of it)
            completion_operands(p, r, multi, ax);
        }
        rec(ev_r(k, R_S), ax);
    }
    // ---- main stream: completion of the local rows of the masked relations (_dfmc.py:319-325), then the two contractions of
    // the G update
    for (size_t k = 0; k < nr; ++k) {
        RelState& r = p->rels[k];
        if (!(dfmc && r.masked)) continue;
        wait(st, ev_r(k, R_S));
        if (r.kn) {                         // the row pass stands for completion + P: A = E T + G_i (S Gram_j S^T)
            if (!r.absent) {
                known_row_pass(p, r, st);
                known_row_dense(p, r, st, false);
            }
        } else if (!r.absent) {
            if (r.mask) complete_masked(p, r, st);
            contraction_P(p, r, st);
        }
        rec(ev_r(k, R_P2), st);
        q_partial(k);
    }
    // ---- second stream: backbones and side products of the unmasked relations, then the side products of the masked ones
    for (size_t k = 0; k < nr; ++k) {
        RelState& r = p->rels[k];
        if (dfmc && r.masked) continue;
        backbone_chain(k);
        side_products(k, ev_r(k, R_WX));
    }
    for (size_t k = 0; k < nr; ++k) {
        RelState& r = p->rels[k];
        if (!(dfmc && r.masked)) continue;
        side_products(k, ev_r(k, R_P2));
    }
    for (size_t i = 0; i < nt; ++i)
        if (!finished[i]) finish_type(i);          // a type without relations: constraints only
    // ---- the next iteration starts behind every gather (and operand refresh)
    for (size_t i = 0; i < nt; ++i) wait(st, ev_t(i, p->bf16 ? T_GT : T_G));
    p->masters_stale = false;
    for (const TypeState& t : p->types) p->masters_stale = p->masters_stale || !t.gather_master;
    p->kn_first = false;
}

// SKF_BF16 plans with owned rows gather only the bf16 operand rows of a type without constraints; at the end of
// skf_iterate_dist every rank fetches the f32 rows of the other owners once, so that skf_get_factor / skf_relation_sqerr see
// the same factors everywhere.
static void finalize_owned(skf_plan* p, hipStream_t st) {
    if (!p->masters_stale) return;
    // on the stream the iteration's exchanges went out on (one communicator, one order of collectives on every rank)
    hipStream_t cs = (owned_can_overlap(p) && p->cs) ? p->cs : st;
    if (cs != st) {
        SKF_HIP(hipEventRecord(p->ev_own[0], st));
        SKF_HIP(hipStreamWaitEvent(cs, p->ev_own[0], 0));
    }
    for (TypeState& t : p->types)
        if (!t.gather_master) collective(p->comm, COLL_ALL_GATHER, t.G.ptr, (size_t)t.chunk * t.c, p->mt, cs);
    if (cs != st) {
        SKF_HIP(hipEventRecord(p->ev_own[1], cs));
        SKF_HIP(hipStreamWaitEvent(st, p->ev_own[1], 0));
    }
    p->masters_stale = false;
}
