// skf_schedule.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): the relation PIPELINE -- the steps of skf_steps.inc ordered over two streams, relation by relation --,
// the three-launch iteration of small graphs, the choice between the schedules (iterate_fit), hipGraph capture, the fold-in.
// ------------------------------------------------------------------------------------------
// The same DFMF iteration as stage_contract + stage_backbone + stage_accumulate, scheduled as a pipeline over
// the relations (whole, unmasked relations; every rank between 65 and 512; MFMA engine): the main stream runs
// nothing but the Gram products and the contractions P_r, Q_r, W_r; everything that follows a relation's
// contractions -- S_r = K_i W_r K_j, the B / D terms, the roundings, its two side products -- runs on the second
// stream UNDERNEATH the contractions of the next relation (those launches leave 60 of the 256 CUs idle when their
// 196 row tiles run unsplit, and every launch has a tail).  Only the last relation's small work, the type-level
// terms G (sum B) and the update itself remain exposed.  Arithmetic and results are those of the staged schedule;
// only the order in which the relations add into E / D differs (relations are walked cheapest-last).
// ------------------------------------------------------------------------------------------
static bool can_pipeline(const skf_plan* p) {
    if (!p->overlap || p->sliced || p->engine != SKF_ENGINE_MFMA || !p->pipeline) return false;
    if (p->variant != SKF_DFMF && p->variant != SKF_DFMC) return false;
    if (p->rels.empty() || p->rels.size() > 64) return false;
    if (!chains_fit_second_stream(p)) return false;      // (every rank <= 64: the one-workgroup chains of the staged schedule)
    if (p->variant == SKF_DFMF)
        for (const TypeState& t : p->types)
            if (t.c <= SMALLC) return false;     // (DFMF: the mixed case stays on the schedule it was measured on)
    for (const RelState& r : p->rels)
        if (r.absent || (r.masked && p->variant != SKF_DFMC)) return false;
    return true;
}

// DFMC adds one dependency to the pipeline: a masked relation is contracted once BEFORE its completion (W = G_i^T R G_j
// of the backbone, _dfmc.py:311-314) and twice after it (_dfmc.py:319-325, 341-345).  Main stream: Gram products; the
// first contraction and W of every masked relation; P, W, Q of the unmasked relations; then completion, P, Q of the
// masked ones -- by then their backbones and reconstruction operands, computed on the second stream underneath the
// unmasked relations' contractions, are long done.
static void iterate_fit_pipelined(skf_plan* p, hipStream_t st) {
    const size_t nt = p->types.size(), nr = p->rels.size();
    hipStream_t ax = p->aux;
    const bool dfmc = (p->variant == SKF_DFMC);
    const int nan_upd = dfmc ? 0 : 1;             // DFMF: nan_to_num on the A/B/C/D terms (_dfmf.py:254-276); DFMC: none (_dfmc.py:127-178)
    if (dfmc && p->first_iter) zero_unknown_entries(p, st);
    p->first_iter = false;
    // per relation: [0] first contraction and W done (main) | [1] backbone and reconstruction operands done (second
    // stream, masked relations) | [2] P done (main) | [3] Q done (main)
    if (p->ev_rel.size() < 4 * nr) {
        const size_t old = p->ev_rel.size();
        p->ev_rel.resize(4 * nr);
        for (size_t k = old; k < 4 * nr; ++k) SKF_HIP(hipEventCreateWithFlags(&p->ev_rel[k], hipEventDisableTiming));
    }
    // order of the relations: most expensive first, so that the exposed tail belongs to the cheapest one
    std::vector<size_t> order(nr);
    for (size_t k = 0; k < nr; ++k) order[k] = k;
    auto cost = [&](size_t k) {
        const RelState& r = p->rels[k];
        return (double)r.nr * (double)p->types[r.col].n * (p->types[r.row].c + p->types[r.col].c);
    };
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cost(a) > cost(b); });

    // ---- main: Gram matrices; second stream: their pseudo-inverses, then the cleared B sums.
    // (Measured, profiles/r02_pipeline_ab.txt: with the Gram products and W = G_i^T P on the second stream as well the
    // contractions slow down by as much as those kernels take -- they are whole-chip launches and any co-resident
    // workgroup takes a CU from them; what the pipeline can hide is what fits on the 60 CUs the unsplit 196-tile
    // launches leave idle and in the launch tails: +1.5 % it/s.)
    // DFMC with a relation kept as lists of its known entries: the main stream opens with the pass over the stored
    // residuals, which is bound by its gathers and leaves the matrix cores idle -- there the Gram products go to the second
    // stream and run BESIDE the pass (config 5: 138.0 -> 140.9 it/s; with the cross-Gram matrices of W there as well, ahead
    // of the pseudo-inverses: 139.1 -- they hold up the chain the row pass waits for; profiles/r03_c5_overlap_ab.txt).
    std::vector<int> all;
    bool any_kn = false;
    for (const RelState& r : p->rels) any_kn = any_kn || r.kn;
    const bool gram_aux = dfmc && any_kn;
    if (gram_aux) {
        SKF_HIP(hipEventRecord(p->ev_fork, st));
        SKF_HIP(hipStreamWaitEvent(ax, p->ev_fork, 0));
    }
    gram_all(p, 1, gram_aux ? ax : st, gram_aux);
    for (size_t i = 0; i < nt; ++i) all.push_back((int)i);
    if (!gram_aux) {
        SKF_HIP(hipEventRecord(p->ev_fork, st));
        SKF_HIP(hipStreamWaitEvent(ax, p->ev_fork, 0));
    }
    // (Round 5, measured and not kept: for DFMC on known-entry lists the pseudo-inverses on the MAIN stream behind the first
    // relation's pass -- here they take 0.78 ms underneath the other relations' passes, 0.2 ms alone; config 5 147.9 against
    // 149.3 it/s: the passes they hold up are worth more than the chains they release.)
    plan_pinv(p, all, ax);
    SKF_HIP(hipMemsetAsync((char*)p->ws_base + p->btot_off, 0, p->btot_bytes, ax));

    std::vector<char> touched(nt, 0);
    std::vector<int> rels_left(nt, 0);           // relations of the type still to come: its sum of B is complete at 0
    for (const RelState& r : p->rels) {
        rels_left[r.row] += 1;
        rels_left[r.col] += 1;
    }
    std::vector<char> updated(nt, 0), has_theta(nt, 0);       // early updates (below): DFMF only, types without constraints
    for (const ThetaState& th : p->thetas) has_theta[th.type] = 1;
    const bool early_ok = !dfmc && p->sw.early_update;
    // type-level terms E_i += G_i sum B-, D_i += G_i sum B+ as soon as the last relation of the type is through
    // (its own launch, added into E / D: the B sums are complete only behind the last relation's backbone)
    auto type_term_of = [&](size_t i) {
        TypeState& t = p->types[i];
        const BSums b = b_sums_master(p, t, ax);
        if (!touched[i]) {                        // a type without relations here: E = D = 0 before the term is added
            SKF_HIP(hipMemsetAsync(t.E.ptr, 0, t.E.bytes, ax));
            SKF_HIP(hipMemsetAsync(t.D.ptr, 0, t.D.bytes, ax));
            touched[i] = 1;
        }
        type_term(p, t, 0, t.n, b.Bn, b.Bp, true, true, ax);
    };
    std::vector<const void*> Sm(nr, nullptr);     // the backbone in the master type, per position in `order`
    // second stream, behind event [0] of the relation: S = K_i W K_j, its B / D terms (paired through T1, which is free
    // once S is there), the rounding of S
    auto backbone_chain = [&](size_t q) {
        RelState& r = p->rels[order[q]];
        SKF_HIP(hipStreamWaitEvent(ax, p->ev_rel[4 * q], 0));
        const bool s32_here = !p->f64 && !p->sw.no_pairs;          // f32 engines: the rounding of S leaves the same launch
        Sm[q] = backbone_general(p, r, nan_upd, s32_here, r.T1.ptr, ax);
        if (!p->f64 && !s32_here) Sm[q] = round_backbone(p, r, ax);
    };
    // second stream: the two side products of the relation behind `ev_p` (P) and event [3] (Q), then the type terms
    auto side_products = [&](size_t q, size_t ev_p) {
        RelState& r = p->rels[order[q]];
        SKF_HIP(hipStreamWaitEvent(ax, p->ev_rel[ev_p], 0));
        if (r.kn) known_row_split(p, r, touched[r.row] != 0, ax);
        else row_side(p, r, true, Sm[q], nullptr, nullptr, false, touched[r.row] != 0, nan_upd, ax);
        touched[r.row] = 1;
        if (--rels_left[r.row] == 0) type_term_of(r.row);         // (before the wait for Q: under the relation's own Q)
        // the type-level term of the column type needs the B sums only (complete with this relation's backbone), not Q:
        // it goes out under the relation's own Q as well, and only the column side product remains behind Q
        const bool last_col = --rels_left[r.col] == 0;
        if (last_col) type_term_of(r.col);
        SKF_HIP(hipStreamWaitEvent(ax, p->ev_rel[4 * q + 3], 0));
        col_side(p, r, true, 0, p->types[r.col].n, Sm[q], nullptr, nullptr, false, touched[r.col] != 0, nan_upd, ax);
        touched[r.col] = 1;
    };

    // ---- masked relations (DFMC), before their completion: the contraction W needs; second stream: backbone, H = G_i S
    for (size_t q = 0; q < nr; ++q) {
        RelState& r = p->rels[order[q]];
        if (!(dfmc && r.masked)) continue;
        const bool by_q = p->types[r.row].c < p->types[r.col].c;      // (W through the narrower factor)
        if (r.kn) {          // known entries only: W from the stored residuals; second stream: backbone, gathered vectors, c x c operands
            // (Measured, profiles/r03_c5_known_entries.txt: on a third stream, beside the matrix-core contractions of the
            // unmasked relations, the pass over the stored residuals just time-slices the chip with them -- 2.0 ms instead
            // of 0.55 ms for user x tag, 92.2 vs 91.6 it/s.  Its 10 000 workgroups leave no CU to share.)
            known_w(p, r, st);
            SKF_HIP(hipEventRecord(p->ev_rel[4 * q], st));
            backbone_chain(q);
            known_operands(p, r, ax, true);
            SKF_HIP(hipEventRecord(p->ev_rel[4 * q + 1], ax));
            continue;
        }
        if (by_q) contraction_Q(p, r, st);
        else contraction_P(p, r, st);
        w_product(p, r, by_q, st);
        SKF_HIP(hipEventRecord(p->ev_rel[4 * q], st));
        backbone_chain(q);
        completion_operands(p, r, true, ax);
        SKF_HIP(hipEventRecord(p->ev_rel[4 * q + 1], ax));
    }
    // ---- unmasked relations: P, W, Q on the main stream.  W goes out between P and Q: the backbone chain and the row
    // side of the relation then run underneath its OWN Q (for the last relation the exposed tail is the column side only).
    // (DFMC: putting the cheap half of them behind the completion block, to shorten the exposed tail, measured equal --
    // their chains are latency-bound and hide better under the large launches; profiles/r02_pipeline_ab.txt.)
    for (size_t q = 0; q < nr; ++q) {
        RelState& r = p->rels[order[q]];
        if (dfmc && r.masked) continue;
        // W through the shorter of the two object dimensions: G_i^T P sums over the rows of the relation, Q^T G_j over its
        // columns (config 3, 100k x 40k: 0.32 -> 0.13 ms).  The Q form has to wait for Q, so the relation's chain then runs
        // under the NEXT relation's contractions instead of its own Q -- not for the last relation, whose tail it would grow.
        const bool w_by_q = (q + 1 < nr) && 5 * p->types[r.col].n <= 3 * r.nr;
        contraction_P(p, r, st);
        if (!w_by_q) {
            w_product(p, r, false, st);
            SKF_HIP(hipEventRecord(p->ev_rel[4 * q], st));
        }
        contraction_Q(p, r, st);
        SKF_HIP(hipEventRecord(p->ev_rel[4 * q + 3], st));
        if (w_by_q) {
            w_product(p, r, true, st);
            SKF_HIP(hipEventRecord(p->ev_rel[4 * q], st));
        }
        backbone_chain(q);
        side_products(q, 4 * q);
        // a type whose last relation this was has its E and D complete behind the side products just issued, and nothing
        // that is still to come reads its factor (no later relation, no constraint on it): its update -- for the bf16 engine
        // also the refresh of the stored G^T -- goes out on the second stream NOW, underneath the remaining relations'
        // contractions, instead of at the exposed end of the iteration (config 3: the 100k-object type, 88 of the 150 us
        // the three updates take).  Same arithmetic, same results.
        if (early_ok)
            for (int side = 0; side < 2; ++side) {
                const size_t i = side == 0 ? (size_t)r.row : (size_t)r.col;
                if (rels_left[i] == 0 && !updated[i] && !has_theta[i] && q + 1 < nr) {
                    update_rows(p, p->types[i], 0, p->types[i].n, ax);
                    updated[i] = 1;
                }
            }
    }
    // ---- masked relations: completion (_dfmc.py:319-325), then the two contractions of the G update
    for (size_t q = 0; q < nr; ++q) {
        RelState& r = p->rels[order[q]];
        if (!(dfmc && r.masked)) continue;
        SKF_HIP(hipStreamWaitEvent(st, p->ev_rel[4 * q + 1], 0));
        if (r.kn) {           // the two residual passes over the lists stand for completion, P and Q
            known_row_pass(p, r, st);
            known_row_dense(p, r, st, false);       // (0.1 ms here; on the low-priority second stream it crawled for 2 ms
                                                    // underneath the column pass and slowed that pass down by 0.4 ms)
            SKF_HIP(hipEventRecord(p->ev_rel[4 * q + 2], st));
            known_col_pass(p, r, st);
            SKF_HIP(hipEventRecord(p->ev_rel[4 * q + 3], st));
            side_products(q, 4 * q + 2);
            continue;
        }
        if (r.mask) complete_masked(p, r, st);
        contraction_P(p, r, st);
        SKF_HIP(hipEventRecord(p->ev_rel[4 * q + 2], st));
        contraction_Q(p, r, st);
        SKF_HIP(hipEventRecord(p->ev_rel[4 * q + 3], st));
        side_products(q, 4 * q + 2);
    }
    for (size_t i = 0; i < nt; ++i)
        if (rels_left[i] == 0 && !touched[i]) type_term_of(i);          // types without relations in this plan
    theta_terms(p, ax);
    SKF_HIP(hipEventRecord(p->ev_join, ax));
    SKF_HIP(hipStreamWaitEvent(st, p->ev_join, 0));
    apply_update(p, st, &updated);
}

// The DFMF iteration of a small graph in three launches (skf_small.h); n_batch > 1: of that many plans of the same graph at
// once -- independent restarts side by side, blockIdx.y = the plan (skf_iterate_batch; p->sm_batch holds their tables)
template <typename T>
static void iterate_small_fused_t(skf_plan* p, hipStream_t st, unsigned n_batch = 1) {
    const SmTables* tb = (const SmTables*)p->sm_tables.ptr;
    const SmTables* const* tbs = (const SmTables* const*)p->sm_batch.ptr;
    constexpr int bb_lds = (2 * 64 + 2 * SM_BK) * SM_LD * 8;
    const SmJob* j1 = (const SmJob*)p->sm_jobs1.ptr;
    const SmJob* j3 = (const SmJob*)p->sm_jobs3.ptr;
    const unsigned n1 = (unsigned)p->sm_j1.size(), n2 = (unsigned)(2 * p->rels.size()), n3 = (unsigned)p->sm_j3.size();
    if (n_batch > 1) {          // restarts side by side: blockIdx.y = the plan
        static DeviceOnce once_c, once_b, once_u;
        allow_dynamic_lds(once_c, small_contract_kernel<T, true>, SM_TILE_BYTES);
        allow_dynamic_lds(once_b, small_backbone_kernel<true>, bb_lds);
        allow_dynamic_lds(once_u, small_update_kernel<T, true>, SM_TILE3_BYTES);
        hipLaunchKernelGGL((small_contract_kernel<T, true>), dim3(n1, n_batch), dim3(256), SM_TILE_BYTES, st, tb, tbs, j1);
        check_launch("small_contract");
        hipLaunchKernelGGL((small_backbone_kernel<true>), dim3(n2, n_batch), dim3(256), bb_lds, st, tb, tbs);
        check_launch("small_backbone");
        hipLaunchKernelGGL((small_update_kernel<T, true>), dim3(n3, n_batch), dim3(256), SM_TILE3_BYTES, st, tb, tbs, j3);
        check_launch("small_update");
    } else {                    // one plan: its tables are the kernel argument
        static DeviceOnce once_c, once_b, once_u;
        allow_dynamic_lds(once_c, small_contract_kernel<T, false>, SM_TILE_BYTES);
        allow_dynamic_lds(once_b, small_backbone_kernel<false>, bb_lds);
        allow_dynamic_lds(once_u, small_update_kernel<T, false>, SM_TILE3_BYTES);
        hipLaunchKernelGGL((small_contract_kernel<T, false>), dim3(n1), dim3(256), SM_TILE_BYTES, st, tb, tbs, j1);
        check_launch("small_contract");
        hipLaunchKernelGGL((small_backbone_kernel<false>), dim3(n2), dim3(256), bb_lds, st, tb, tbs);
        check_launch("small_backbone");
        hipLaunchKernelGGL((small_update_kernel<T, false>), dim3(n3), dim3(256), SM_TILE3_BYTES, st, tb, tbs, j3);
        check_launch("small_update");
    }
    p->first_iter = false;
}

static void iterate_fit(skf_plan* p, hipStream_t st) {
    if (p->small_fused) {
        if (p->f64) iterate_small_fused_t<double>(p, st);
        else iterate_small_fused_t<float>(p, st);
        return;
    }
    if (can_pipeline(p)) {
        iterate_fit_pipelined(p, st);
        return;
    }
    accumulate_fit(p, st);
    apply_update(p, st);
}

static bool use_graph(skf_plan* p, hipStream_t st, int n_iters) {
    if (st == nullptr || p->profiling || p->graph_failed || n_iters < 4 || !p->mon.lists.empty()) return false;
    // opt-in (SKF_GRAPH=1): measured on dicty (50 launches / 0.5 ms iteration) the replay is not
    // faster than the asynchronous eager launches -- the iteration is bound by kernel time
    return p->graph_on || p->sw.graph;
}

// Record one iteration into a hipGraph (the second-stream fork/join becomes graph edges).
// Any failure leaves the plan on the eager path.
static void capture_iteration(skf_plan* p, hipStream_t st) {
    if (p->graph_exec) {
        (void)hipGraphExecDestroy(p->graph_exec);
        p->graph_exec = nullptr;
    }
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        p->graph_failed = true;
        return;
    }
    hipGraph_t graph = nullptr;
    bool ok = true;
    try {
        iterate_fit(p, st);
    } catch (const Error&) {
        ok = false;
    }
    if (hipStreamEndCapture(st, &graph) != hipSuccess || !ok || graph == nullptr) {
        (void)hipGetLastError();
        if (graph) (void)hipGraphDestroy(graph);
        p->graph_failed = true;
        return;
    }
    if (hipGraphInstantiate(&p->graph_exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        p->graph_exec = nullptr;
        p->graph_failed = true;
    }
    (void)hipGraphDestroy(graph);
    p->graph_stream = st;
}

// SKF_TRANSFORM: everything that does not depend on G_target is computed once.
static void prepare_transform(skf_plan* p, hipStream_t st) {
    TypeState& tt = p->types[p->target];
    SKF_HIP(hipMemsetAsync(tt.Ec.ptr, 0, tt.Ec.bytes, st));
    SKF_HIP(hipMemsetAsync(tt.Dc.ptr, 0, tt.Dc.bytes, st));
    SKF_HIP(hipMemsetAsync(tt.Bp_tot.ptr, 0, tt.Bp_tot.bytes, st));
    SKF_HIP(hipMemsetAsync(tt.Bn_tot.ptr, 0, tt.Bn_tot.bytes, st));
    for (size_t i = 0; i < p->types.size(); ++i)
        if ((int)i != p->target) gram(p, p->types[i], 0, st);
    for (RelState& r : p->rels) {
        TypeState& ti = p->types[r.row];
        TypeState& tj = p->types[r.col];
        const int ni = (int)ti.n, nj = (int)tj.n, ci = ti.c, cj = tj.c;
        if (r.fold) {                         // the stored entries, compressed along the target: T = G_p S', one pass into Ec / Dc
            if (!r.fold_known) fold_prepare(p, r, st);
            const bool row_side = r.row == p->target;
            relation_small_terms(p, r, 0, EPI_SPLIT_ACC, row_side ? tt.Bp_tot.ptr : nullptr, row_side ? tt.Bn_tot.ptr : nullptr,
                                 row_side ? nullptr : tt.Bp_tot.ptr, row_side ? nullptr : tt.Bn_tot.ptr, row_side, !row_side, st);
            if (r.fold_known) fold_known_prepare(p, r, st);      // (stored = known: T and the unsplit B_r, nothing into Ec / Dc)
            continue;
        }
        if (r.row == p->target) {             // _dfmf.py:392-405
            GemmArgs g = gemm_args(r.R, r.ldr, 1, tj.G.ptr, cj, 1, r.P.ptr, cj, ni, cj, nj, EPI_STORE, 0);
            relation_gemm(p, g, st, &r, false);
            g = gemm_args(r.P.ptr, cj, 1, r.S.ptr, 1, cj, tt.Ec.ptr, ci, ni, ci, cj, EPI_SPLIT_ACC, 0);
            g.C2 = tt.Dc.ptr;
            mixed_gemm(p, g, st);
            relation_small_terms(p, r, 0, EPI_SPLIT_ACC, tt.Bp_tot.ptr, tt.Bn_tot.ptr, nullptr, nullptr, true,
                                 false, st);
        } else {                              // _dfmf.py:407-419
            GemmArgs g = gemm_args(r.R, 1, r.ldr, ti.G.ptr, ci, 1, r.Q.ptr, ci, nj, ci, ni, EPI_STORE, 0);
            relation_gemm(p, g, st, &r, true);
            g = gemm_args(r.Q.ptr, ci, 1, r.S.ptr, cj, 1, tt.Ec.ptr, cj, nj, cj, ci, EPI_SPLIT_ACC, 0);
            g.C2 = tt.Dc.ptr;
            mixed_gemm(p, g, st);
            relation_small_terms(p, r, 0, EPI_SPLIT_ACC, nullptr, nullptr, tt.Bp_tot.ptr, tt.Bn_tot.ptr, false,
                                 true, st);
        }
    }
    p->prepared = true;
}

// The fold-in iteration as ONE launch (foldin_step_kernel): no constraint on the target type (a constraint couples the
// rows of an iteration through E / D, which this form never writes)
static bool fold_fused(const skf_plan* p) {
    // (a SKF_REL_FOLD_KNOWN relation reads the moving factor through its lists every iteration: the unfused path below)
    return p->variant == SKF_TRANSFORM && p->engine == SKF_ENGINE_MFMA && p->thetas.empty() && !p->fold_x.bytes;
}

// `iters` fold-in iterations of `n_plans` plans of one graph (same object count and rank of the target), every launch
// serving all of them; each plan's factor ends in its G slot (the two buffers swap roles per launch)
static void fold_steps(skf_plan* const* plans, int n_plans, int iters, hipStream_t st) {
    skf_plan* p0 = plans[0];
    const TypeState& t0 = p0->types[p0->target];
    for (int b0 = 0; b0 < n_plans; b0 += FOLD_MAXB) {
        const int nb = n_plans - b0 < FOLD_MAXB ? n_plans - b0 : FOLD_MAXB;
        for (int it = 0; it < iters; ++it) {
            FoldArgs a;
            memset(&a, 0, sizeof a);
            a.n = (int)t0.n; a.c = t0.c;
            for (int k = 0; k < nb; ++k) {
                TypeState& t = plans[b0 + k]->types[plans[b0 + k]->target];
                a.G[k] = t.G.ptr; a.Gout[k] = t.Galt.ptr;
                a.Bn[k] = t.Bn_tot.ptr; a.Bp[k] = t.Bp_tot.ptr;
                a.Ec[k] = t.Ec.ptr; a.Dc[k] = t.Dc.ptr;
            }
            if (p0->f64) {
                if (t0.n > 64 && t0.c > 64) {
                    dim3 grid(cdiv(t0.c, 64), cdiv(t0.n, 64), nb);
                    hipLaunchKernelGGL((foldin_step_kernel<double, 2, 2, 16>), grid, dim3(GEMM_THREADS), 0, st, a);
                } else {
                    dim3 grid(cdiv(t0.c, 32), cdiv(t0.n, 32), nb);
                    hipLaunchKernelGGL((foldin_step_kernel<double, 1, 1, 16>), grid, dim3(GEMM_THREADS), 0, st, a);
                }
            } else {
                dim3 grid(cdiv(t0.c, 64), cdiv(t0.n, 64), nb);
                hipLaunchKernelGGL((foldin_step_kernel<float, 1, 1, 16>), grid, dim3(GEMM_THREADS), 0, st, a);
            }
            check_launch("foldin_step");
            for (int k = 0; k < nb; ++k) {
                TypeState& t = plans[b0 + k]->types[plans[b0 + k]->target];
                std::swap(t.G.ptr, t.Galt.ptr);
                std::swap(t.G.off, t.Galt.off);
            }
        }
    }
}

static void iterate_transform(skf_plan* p, hipStream_t st) {
    if (fold_fused(p)) {
        skf_plan* one[1] = {p};
        fold_steps(one, 1, 1, st);
        return;
    }
    TypeState& tt = p->types[p->target];
    const int n = (int)tt.n, c = tt.c;
    SKF_HIP(hipMemcpyAsync(tt.E.ptr, tt.Ec.ptr, tt.E.bytes, hipMemcpyDeviceToDevice, st));
    SKF_HIP(hipMemcpyAsync(tt.D.ptr, tt.Dc.ptr, tt.D.bytes, hipMemcpyDeviceToDevice, st));
    for (RelState& r : p->rels)              // stored = known: the split of this relation's tmp1, in relation order
        if (r.fold_known) fold_known_step(p, r, st);
    GemmArgs g = gemm_args(tt.G.ptr, c, 1, tt.Bn_tot.ptr, c, 1, tt.E.ptr, c, n, c, c, EPI_ACC, 0);
    mixed_gemm(p, g, st);
    g = gemm_args(tt.G.ptr, c, 1, tt.Bp_tot.ptr, c, 1, tt.D.ptr, c, n, c, c, EPI_ACC, 0);
    mixed_gemm(p, g, st);
    theta_terms(p, st);
    mult_update(p, tt, st);
    if (!p->thetas.empty()) refresh_gt(p, tt, st);      // SKF_BF16: the constraint products read the stored G^T
}
