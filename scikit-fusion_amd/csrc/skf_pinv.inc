// skf_pinv.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): the host side of the pseudo-inverse K = pinv(Gram) (kernels: skf_pinv.h).  ONE route cascade, run_pinv,
// that its two callers describe a pass to: plan_pinv (every schedule of a plan) and skf_pinv_sym (the stand-alone operator,
// skf_api.hip; its workspace layout: pinv_sym_layout).
//   pack -> blocked sweep (writes K) | Cholesky inverse + unpack -> deflation over several workgroups (orders above
//   SWEEP_MAXN) -> deflation in one workgroup -> Jacobi eigen-solver -> eigen unpack
// Every launch behind the fast path is gated on the device by the verdict words (EighArgs::chol_ok): no host round trip.

// Relative pivot threshold of the Cholesky fast path: below it the Gram matrix goes to the deflation / the
// eigen-solver.  SKF_PINV_JACOBI=1 forces the eigen path with its exact singular-value cut-off (tests).
static double chol_rel_threshold(const Switches& sw) { return sw.pinv_jacobi ? 1e300 : 1e-8; }
// lower edge of the deflation's gap test
static double deflation_lo(const Switches& sw) { return sw.pinv_jacobi ? 1e300 : 1e-10; }

// Cholesky fast path: the LDS-blocked kernel up to order CHOLB_MAXN, the plain one beyond
static void launch_chol(const Switches& sw, const EighArgs& e, int batch, int max_order, hipStream_t st) {
    if (max_order <= CHOLS_MAXN && !sw.chol_no_small && !sw.chol_unblocked) {
        hipLaunchKernelGGL(chol_inverse_small_kernel, dim3((unsigned)batch), dim3(64), 0, st, e, chol_rel_threshold(sw));
    } else if (max_order <= CHOLB_MAXN && !sw.chol_unblocked) {
        size_t wave_tiles = (size_t)(EIGH_THREADS / 64) * CHOLB_NB * (CHOLB_NB + 1);
        size_t panel = (size_t)CHOLB_NB * max_order;
        size_t smem = ((size_t)CHOLB_NB * (CHOLB_NB + 1) + (panel > wave_tiles ? panel : wave_tiles)) * sizeof(double);
        static DeviceOnce once;
        allow_dynamic_lds(once, chol_inverse_blocked_kernel,
                          (int)(((size_t)CHOLB_NB * (CHOLB_NB + 1) + (size_t)CHOLB_NB * CHOLB_MAXN) * sizeof(double)));
        hipLaunchKernelGGL(chol_inverse_blocked_kernel, dim3((unsigned)batch), dim3(EIGH_THREADS), smem, st, e,
                           chol_rel_threshold(sw));
    } else {
        hipLaunchKernelGGL(chol_inverse_kernel, dim3((unsigned)batch), dim3(EIGH_THREADS), 0, st, e, chol_rel_threshold(sw));
    }
    check_launch("chol_inverse");
}

// The blocked sweep of `nb` matrices of order <= max_c: from order sw.sweep_step_min (default: always) one launch per block
// step with the rank-32 update of the step spread over row slabs -- orders up to SWEEP_MAXN with the panel in LDS, up to
// EIGH_MAXN with the column operands from memory --, else (orders <= SWEEP_MAXN) one workgroup per matrix in one launch.
static bool sweep_steps(const Switches& sw, int max_c) { return sw.sweep_step_min > 0 && max_c >= sw.sweep_step_min; }
static bool sweep_takes(const Switches& sw, int max_c) {
    if (max_c <= CHOLS_MAXN || sw.no_sweep || sw.chol_unblocked || sw.pinv_jacobi) return false;
    return max_c <= SWEEP_MAXN || (sweep_steps(sw, max_c) && max_c <= EIGH_MAXN && !sw.no_sweep_big);
}
static void launch_sweep(const Switches& sw, const EighArgs& e, const PinvBatch& pb, int nb, int max_c, hipStream_t st) {
    if (sweep_steps(sw, max_c)) {
        const bool big = max_c > SWEEP_MAXN;
        static DeviceOnce once, once_big;
        if (big) allow_dynamic_lds(once_big, sweep_step_kernel<true>, SWEEP_BIG_LDS_BYTES);
        else allow_dynamic_lds(once, sweep_step_kernel<false>, SWEEP_LDS_BYTES);
        const int rs = big ? SWEEP_NB : sw.sweep_rows;
        const int slabs = (max_c + rs - 1) / rs, steps = (max_c + SWEEP_NB - 1) / SWEEP_NB;
        for (int step = 0; step < steps; ++step) {
            if (big)
                hipLaunchKernelGGL(sweep_step_kernel<true>, dim3((unsigned)nb, (unsigned)slabs), dim3(SWEEP_THREADS), SWEEP_BIG_LDS_BYTES, st,
                                   e, pb, chol_rel_threshold(sw), step, rs);
            else
                hipLaunchKernelGGL(sweep_step_kernel<false>, dim3((unsigned)nb, (unsigned)slabs), dim3(SWEEP_THREADS), SWEEP_LDS_BYTES, st, e,
                                   pb, chol_rel_threshold(sw), step, rs);
            check_launch("sweep_step");
        }
        return;
    }
    static DeviceOnce once;
    allow_dynamic_lds(once, sweep_inverse_kernel, SWEEP_LDS_BYTES);
    hipLaunchKernelGGL(sweep_inverse_kernel, dim3((unsigned)nb), dim3(SWEEP_THREADS), SWEEP_LDS_BYTES, st, e, pb, chol_rel_threshold(sw));
    check_launch("sweep_inverse");
}

// Rank-revealing deflation over several workgroups (skf_pinv.h, pchol_step_kernel) for the matrices of a batch whose fast
// path failed, orders above SWEEP_MAXN: every launch is gated on the device (chol_ok, the verdict of the steps, the verdict of
// the sweep over B), the host issues the sequence blind.  K[b]: c x c f64, ld = c.  `scratch`: defl_scratch_bytes(nb, stride).
static size_t defl_scratch_bytes(int nb, int64_t stride) {
    return align_up((size_t)3 * nb * stride * 8, 256) + align_up((size_t)nb * 2 * EIGH_MAXN * 8, 256) +
           align_up((size_t)nb * 4 * 8, 256) + align_up((size_t)nb * 8 * sizeof(int), 256);
}
static bool defl_multi_takes(const Switches& sw, int max_c) {
    return max_c > SWEEP_MAXN && max_c < EIGH_MAXN && sweep_takes(sw, max_c) && !sw.pinv_jacobi;
}
static void launch_deflation_multi(const Switches& sw, int engine, const EighArgs& e, const PinvBatch& pb, int nb, int max_c,
                                   void* scratch, hipStream_t st) {
    char* base = (char*)scratch;
    double* M0 = (double*)base;
    double* M1 = M0 + (size_t)nb * e.stride;
    double* Binv = M1 + (size_t)nb * e.stride;
    base += align_up((size_t)3 * nb * e.stride * 8, 256);
    DeflArgs da;
    da.d = (double*)base;
    base += align_up((size_t)nb * 2 * EIGH_MAXN * 8, 256);
    da.vals = (double*)base;
    base += align_up((size_t)nb * 4 * 8, 256);
    da.state = (int*)base;
    da.n_defl = da.state + 4 * nb;
    da.gate = da.n_defl + nb;
    da.ok2 = da.gate + nb;
    da.rank = da.ok2 + nb;
    const int np = max_c + (max_c & 1);
    hipLaunchKernelGGL(pchol_init_kernel, dim3(elem_grid((int64_t)np * np), (unsigned)nb), dim3(256), 0, st, e, da);
    check_launch("pchol_init");
    const int steps = 2 * cdiv(max_c, DEFL_NB) + 1, slabs = cdiv(max_c, DEFL_ROWS);
    for (int step = 0; step < steps; ++step) {
        hipLaunchKernelGGL(pchol_step_kernel, dim3((unsigned)nb, (unsigned)slabs), dim3(DEFL_THREADS), 0, st, e, da, deflation_lo(sw), 1e-7,
                           step);
        check_launch("pchol_step");
    }
    const int fin = steps & 1;
    hipLaunchKernelGGL(pchol_verdict_kernel, dim3((unsigned)nb), dim3(64), 0, st, e, da, fin);
    check_launch("pchol_verdict");
    const GemmTypes f64{SKF_F64, SKF_F64, SKF_F64};
    for (int b = 0; b < nb; ++b) {                      // B = L^T L  (Lt[k][i] = L[i][k], ld = the padded order)
        const int c = pb.c[b], ld = pb.n_pad[b];
        const double* Lt = e.V + (int64_t)b * e.stride;
        GemmArgs g = gemm_args(Lt, ld, 1, Lt, 1, ld, e.Vs + (int64_t)b * e.stride, ld, c, c, c, EPI_STORE, 0);
        g.gate = da.gate + b;
        run_gemm(f64, engine, g, 1, nullptr, 0, st);
    }
    hipLaunchKernelGGL(pchol_patch_kernel, dim3((unsigned)nb), dim3(256), 0, st, e, da, fin);
    check_launch("pchol_patch");
    {                                                   // B^-1 by the blocked sweep of the fast path (idle where n_defl = 0)
        EighArgs e2 = e;
        e2.A = e.Vs; e2.V = M0; e2.Vs = M1;
        e2.n_orig = da.n_defl;
        e2.chol_ok = da.ok2;
        PinvBatch pb2 = pb;
        for (int b = 0; b < nb; ++b) pb2.K[b] = Binv + (int64_t)b * e.stride;
        launch_sweep(sw, e2, pb2, nb, max_c, st);
    }
    hipLaunchKernelGGL(pchol_gate2_kernel, dim3((unsigned)nb), dim3(64), 0, st, da);
    check_launch("pchol_gate2");
    for (int b = 0; b < nb; ++b) {
        const int c = pb.c[b], ld = pb.n_pad[b];
        const double* Lt = e.V + (int64_t)b * e.stride;
        const double* Bi = Binv + (int64_t)b * e.stride;        // (the sweep writes its result with ld = the order)
        double* Yt = M0 + (int64_t)b * e.stride;
        GemmArgs g = gemm_args(Bi, c, 1, Lt, ld, 1, Yt, ld, c, c, c, EPI_STORE, 0);         // Y^T = B^-1 L^T
        g.gate = da.gate + b;
        run_gemm(f64, engine, g, 1, nullptr, 0, st);
        g = gemm_args(Yt, 1, ld, Yt, ld, 1, pb.K[b], c, c, c, c, EPI_STORE, 0);             // K = Y Y^T
        g.gate = da.gate + b;
        run_gemm(f64, engine, g, 1, nullptr, 0, st);
    }
    hipLaunchKernelGGL(pchol_done_kernel, dim3((unsigned)nb), dim3(64), 0, st, e, da);
    check_launch("pchol_done");
}
// One pseudo-inverse pass over `nb` matrices, as its caller describes it.
struct PinvRun {
    const Switches* sw;
    int engine;                 // of the products inside the multi-workgroup deflation
    EighArgs e;                 // the eigen workspace of all nb matrices
    const PinvBatch* pb;        // the caller's matrices in chunks of up to PINV_MAXB: cdiv(nb, PINV_MAXB) of them
    int nb, max_c, max_pad;     // matrix count, largest order, largest padded order
    int lds_order;              // the order that sizes the LDS of the Cholesky kernels and of pchol_pinv_kernel
    int dtype;                  // element type of the caller's matrices: SKF_F64 / SKF_F32
    bool k_direct;              // every K is f64 with ld = c: the sweep and the multi-workgroup deflation may write it themselves
    void* defl_scratch;         // defl_scratch_bytes(nb, e.stride) for the multi-workgroup deflation, or null
    bool write_orders;          // the pack writes e.n / e.n_orig (no bind step has uploaded them)
};

// a pack / unpack launch per chunk of up to PINV_MAXB matrices (pointers travel as kernel arguments), in the caller's
// element type: launch(T(), chunk, first matrix, matrices)
template <class F>
static void pinv_chunks(const PinvRun& r, F&& launch) {
    for (int b0 = 0; b0 < r.nb; b0 += PINV_MAXB) {
        const int n = std::min(PINV_MAXB, r.nb - b0);
        if (r.dtype == SKF_F64) launch(double(), r.pb[b0 / PINV_MAXB], b0, n);
        else launch(float(), r.pb[b0 / PINV_MAXB], b0, n);
    }
}

static void run_pinv(const PinvRun& r, hipStream_t st) {
    const Switches& sw = *r.sw;
    const EighArgs& e = r.e;
    const bool batched = r.nb <= PINV_MAXB;     // sweep and multi-workgroup deflation take their pointers from ONE PinvBatch
    pinv_chunks(r, [&](auto t, const PinvBatch& pb, int b0, int n) {
        hipLaunchKernelGGL((eigh_pack_kernel<decltype(t)>), dim3(elem_grid((int64_t)r.max_pad * r.max_pad), n), dim3(256), 0, st, pb,
                           e.A + (int64_t)b0 * e.stride, e.stride, r.write_orders ? (int*)e.n + b0 : nullptr,
                           r.write_orders ? (int*)e.n_orig + b0 : nullptr);
        check_launch("eigh_pack");
    });
    // fast path with an on-device verdict; the deflations and the Jacobi eigen-solver only do work for the matrices the
    // fast path rejected -- no host round trip either way.  Orders 65 .. 256 (round 4), up to EIGH_MAXN (round 5): the
    // blocked sweep operator writes K itself -- one launch instead of the Cholesky inverse and its unpack (1.15 + 0.09 ms
    // at order 256)
    if (batched && r.k_direct && sweep_takes(sw, r.max_c)) {
        launch_sweep(sw, e, r.pb[0], r.nb, r.max_c, st);
    } else {
        launch_chol(sw, e, r.nb, r.lds_order, st);
        pinv_chunks(r, [&](auto t, const PinvBatch& pb, int b0, int n) {
            hipLaunchKernelGGL((chol_unpack_kernel<decltype(t)>), dim3(elem_grid((int64_t)r.max_c * r.max_c), n), dim3(256), 0, st, pb,
                               (const double*)e.V + (int64_t)b0 * e.stride, e.stride, (const int*)e.chol_ok + b0);
            check_launch("chol_unpack");
        });
    }
    // the matrices the fast path declined (verdicts in e.chol_ok, packed copies in e.A); no-ops for the others.
    // Orders above 256: the deflation over several workgroups first (round 6); what it declines is still there for the rest
    if (batched && r.k_direct && r.defl_scratch && r.engine == SKF_ENGINE_MFMA && defl_multi_takes(sw, r.max_c))
        launch_deflation_multi(sw, r.engine, e, r.pb[0], r.nb, r.max_c, r.defl_scratch, st);
    // a rank-deficient Gram matrix with a clear spectral gap: rank-revealing deflation (pchol_pinv_kernel); what it
    // declines goes to the eigen-solver with the exact singular-value cut-off
    {
        static DeviceOnce once;
        allow_dynamic_lds(once, pchol_pinv_kernel, PCHOL_LDS_BYTES);
    }
    {   // dynamic LDS for the packed factor of L^T L, sized by the largest order the workspace was laid out for (a no-op
        // launch still has to find a CU with that much LDS free, so small graphs reserve little)
        const int lr = r.lds_order < PCHOL_LDS_R ? r.lds_order : PCHOL_LDS_R;
        hipLaunchKernelGGL(pchol_pinv_kernel, dim3((unsigned)r.nb), dim3(EIGH_THREADS), (size_t)lr * (lr + 1) / 2 * 8, st, e,
                           deflation_lo(sw), 1e-7, lr);
    }
    check_launch("pchol_pinv");
    hipLaunchKernelGGL(jacobi_eigh_kernel, dim3((unsigned)r.nb), dim3(EIGH_THREADS), 0, st, e);
    check_launch("jacobi_eigh");
    pinv_chunks(r, [&](auto t, const PinvBatch& pb, int b0, int n) {
        hipLaunchKernelGGL((eigh_unpack_pinv_kernel<decltype(t)>), dim3(elem_grid((int64_t)r.max_c * r.max_c), n), dim3(256), 0, st, pb,
                           (const double*)e.Vs + (int64_t)b0 * e.stride, (const double*)e.V + (int64_t)b0 * e.stride, e.stride,
                           (const int*)e.chol_ok + b0);
        check_launch("eigh_unpack");
    });
}

// K_i = pinv(Gram_i) for every type (one workgroup each); `which` = 0..n_types-1, the order
// of the per-matrix order arrays uploaded once by skf_plan_bind_workspace.
static void plan_pinv(skf_plan* p, const std::vector<int>& which, hipStream_t st) {
    if (which.empty()) return;
    PinvRun r;
    r.sw = &p->sw; r.engine = p->engine;
    r.e.A = (double*)p->eigA.ptr; r.e.V = (double*)p->eigV.ptr; r.e.Vs = (double*)p->eigVs.ptr;
    r.e.w = (double*)p->eigW.ptr; r.e.stride = p->eig_stride; r.e.wstride = p->eig_maxn;
    r.e.n = (const int*)p->eigN.ptr; r.e.n_orig = (const int*)p->eigNorig.ptr;
    r.e.chol_ok = (int*)p->eigOk.ptr;
    r.e.max_sweeps = 30;
    r.nb = (int)which.size(); r.max_c = 1; r.max_pad = 2;
    std::vector<PinvBatch> pb((size_t)cdiv(r.nb, PINV_MAXB));
    for (int b = 0; b < r.nb; ++b) {
        const TypeState& t = p->types[which[b]];
        PinvBatch& q = pb[b / PINV_MAXB];
        const int k = b % PINV_MAXB;
        q.gram[k] = t.Gram.ptr; q.ldg[k] = t.c;
        q.K[k] = t.K.ptr; q.ldk[k] = t.c;
        q.c[k] = t.c; q.n_pad[k] = t.n_pad;
        if (t.n_pad > r.max_pad) r.max_pad = t.n_pad;
        if (t.c > r.max_c) r.max_c = t.c;
    }
    r.pb = pb.data();
    r.lds_order = p->eig_maxn;
    r.dtype = SKF_F64;                  // the c x c algebra of every engine
    r.k_direct = true;
    r.defl_scratch = p->eigX.ptr;       // (plan_layout: plans with an order above SWEEP_MAXN and at most PINV_MAXB types)
    r.write_orders = false;
    run_pinv(r, st);
}

// Workspace of the stand-alone operator skf_pinv_sym, byte offsets: three n_pad^2 f64 matrices, the eigenvalue row, the int
// words (padded order, order at +16 words, verdict at +32), then -- orders above SWEEP_MAXN -- the scratch of the
// multi-workgroup deflation.
struct PinvSymLayout {
    size_t A, V, Vs, w, n, n_orig, ok, defl, total;
};
static PinvSymLayout pinv_sym_layout(int n) {
    const size_t np = (size_t)(n + 1) / 2 * 2, mat = align_up(np * np * 8, 256);
    PinvSymLayout l;
    l.A = 0; l.V = mat; l.Vs = 2 * mat; l.w = 3 * mat;
    l.n = 3 * mat + align_up(np * 8, 256); l.n_orig = l.n + 16 * sizeof(int); l.ok = l.n + 32 * sizeof(int);
    l.defl = l.total = l.n + 512;
    if (n > SWEEP_MAXN) l.total += defl_scratch_bytes(1, (int64_t)np * np) + 256;
    return l;
}
