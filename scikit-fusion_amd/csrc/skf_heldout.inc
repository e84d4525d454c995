// skf_heldout.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): held-out pairs scored inside the fit -- the checks, the layout of the monitor's workspace, the
// launches of one evaluation (H = G_i S through the plan's product wrappers, the pass, the judge, the snapshot) and the C
// entry points.  Kernels: skf_heldout.h; the state a monitored plan carries: HeldoutMonitor (skf_plan.inc).
//
// Workspace of a monitor (every part 256-byte aligned; nothing of size n_i x n_j):
//   state words 256 B | first partial of every list | totals of the last evaluation | snapshot ranges | slab partials of
//   every list | per list: H = G_i S (n_i x c_j, master type) and the split-K scratch of that product | history
//   capacity x n_lists f64 | one snapshot of every factor master and every backbone

static inline bool monitored(const skf_plan* p) { return !p->mon.lists.empty(); }

// H = G_i S of a held-out list's relation: master x f64 -> master, the product kind of sqerr_stored's H
static GemmArgs heldout_product(const skf_plan* p, const RelState& r, void* H) {
    const TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    return gemm_args(ti.G.ptr, ti.c, 1, r.S.ptr, tj.c, 1, H, tj.c, (int)ti.n, tj.c, ti.c, EPI_STORE, 0);
}

struct HeldoutLayout {
    size_t state = 0, offs = 0, cur = 0, segs = 0, partials = 0, history = 0, total = 0;
    std::vector<size_t> H, part, part_bytes, snap_g, snap_s;
    std::vector<int64_t> blocks;
};

// what skf_plan_heldout_workspace_bytes and skf_plan_set_heldout both check, from the host-side fields alone
static void heldout_check_plan(const skf_plan* p, int32_t n_lists, const skf_heldout_desc* d, int64_t capacity) {
    if (!p) SKF_FAIL(SKF_E_INVALID, "null plan");
    if (n_lists < 0 || (n_lists > 0 && !d)) SKF_FAIL(SKF_E_INVALID, "held-out lists: bad count / null descriptors");
    if (capacity < 0) SKF_FAIL(SKF_E_INVALID, "held-out lists: capacity_iters %lld is negative", (long long)capacity);
    if (p->variant == SKF_TRANSFORM) SKF_FAIL(SKF_E_INVALID, "held-out lists: SKF_DFMF / SKF_DFMC plans only");
    if (p->sliced || p->owned || p->comm) SKF_FAIL(SKF_E_INVALID, "held-out lists: not for plans with row blocks, owned rows or a communicator");
    for (int l = 0; l < n_lists; ++l) {
        if (d[l].rel < 0 || d[l].rel >= (int)p->rels.size()) SKF_FAIL(SKF_E_INVALID, "held-out list %d: relation %d out of range", l, d[l].rel);
        if (d[l].n < 1 || d[l].n >= (1LL << 40)) SKF_FAIL(SKF_E_INVALID, "held-out list %d (relation %d): n = %lld, at least one pair is needed", l, d[l].rel, (long long)d[l].n);
        if (!d[l].rows || !d[l].cols || !d[l].values) SKF_FAIL(SKF_E_INVALID, "held-out list %d (relation %d): null pointer", l, d[l].rel);
        for (int q = 0; q < l; ++q)
            if (d[q].rel == d[l].rel) SKF_FAIL(SKF_E_INVALID, "held-out lists %d and %d both name relation %d: at most one list per relation", q, l, d[l].rel);
        const RelState& r = p->rels[d[l].rel];
        if (r.absent || r.nr != p->types[r.row].n) SKF_FAIL(SKF_E_INVALID, "held-out list %d: relation %d is not held whole here", l, d[l].rel);
        if (p->types[r.col].c > 1024) SKF_FAIL(SKF_E_INVALID, "held-out list %d (relation %d): rank %d of the column type above 1024", l, d[l].rel, p->types[r.col].c);
    }
}

static HeldoutLayout heldout_layout(const skf_plan* p, int32_t n_lists, const skf_heldout_desc* d, int64_t capacity) {
    HeldoutLayout L;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align_up(bytes ? bytes : 1, 256); return o; };
    L.state = take(256);
    L.offs = take(((size_t)n_lists + 1) * 8);
    L.cur = take((size_t)n_lists * 8);
    L.segs = take((p->types.size() + p->rels.size()) * sizeof(HeldoutSeg));
    size_t blocks = 0;
    for (int l = 0; l < n_lists; ++l) {
        L.blocks.push_back((d[l].n + HELDOUT_SLAB - 1) / HELDOUT_SLAB);
        blocks += (size_t)L.blocks.back();
    }
    L.partials = take(blocks * 8);
    for (int l = 0; l < n_lists; ++l) {
        const RelState& r = p->rels[d[l].rel];
        const TypeState &ti = p->types[r.row], &tj = p->types[r.col];
        L.H.push_back(take((size_t)ti.n * tj.c * p->esz));
        L.part_bytes.push_back(kind_part_bytes(p, kind_mixed(p), ti.n, tj.c, ti.c));
        L.part.push_back(take(L.part_bytes.back()));
    }
    L.history = take((size_t)capacity * n_lists * 8);
    for (const TypeState& t : p->types) L.snap_g.push_back(take((size_t)t.n * t.c * p->esz));
    for (const RelState& r : p->rels) L.snap_s.push_back(take((size_t)p->types[r.row].c * p->types[r.col].c * 8));
    L.total = at;
    return L;
}

static void heldout_check_ready(const skf_plan* p, const char* what) {
    if (!p) SKF_FAIL(SKF_E_INVALID, "null plan");
    if (!p->bound) SKF_FAIL(SKF_E_STATE, "workspace not bound");
    if (!monitored(p)) SKF_FAIL(SKF_E_STATE, "%s: no held-out lists attached (skf_plan_set_heldout)", what);
}

// One evaluation under the current (G, S): per list the product and the pass, then the judge -- `judge`: with the state
// words, the history row and the snapshot; without: the totals only (cur).
static void heldout_eval(skf_plan* p, bool judge, hipStream_t st) {
    HeldoutMonitor& m = p->mon;
    int64_t first = 0;
    for (const HeldoutList& hl : m.lists) {
        const RelState& r = p->rels[hl.rel];
        const TypeState& tj = p->types[r.col];
        const ProductKind k = kind_mixed(p);
        run_gemm(k.ty, p->engine, heldout_product(p, r, hl.H), 0, hl.part, hl.part_bytes, st, k.relation);
        if (p->f64)
            hipLaunchKernelGGL((heldout_sqerr_kernel<double>), dim3((unsigned)hl.blocks), dim3(HELDOUT_THREADS), 0, st, (const double*)hl.H,
                               (int64_t)tj.c, (const double*)tj.G.ptr, (int64_t)tj.c, tj.c, hl.rows, hl.cols, (const double*)hl.vals, hl.n,
                               m.partials + first);
        else
            hipLaunchKernelGGL((heldout_sqerr_kernel<float>), dim3((unsigned)hl.blocks), dim3(HELDOUT_THREADS), 0, st, (const float*)hl.H,
                               (int64_t)tj.c, (const float*)tj.G.ptr, (int64_t)tj.c, tj.c, hl.rows, hl.cols, (const float*)hl.vals, hl.n,
                               m.partials + first);
        check_launch("heldout_sqerr");
        first += hl.blocks;
    }
    hipLaunchKernelGGL(heldout_judge_kernel, dim3(1), dim3(256), 0, st, (const double*)m.partials, (const int64_t*)m.offs, (int)m.lists.size(),
                       m.cur, judge ? m.state : (HeldoutState*)nullptr, m.history, m.capacity, m.patience, m.min_delta);
    check_launch("heldout_judge");
    if (judge) {
        int64_t gx = (m.max_words / 4 + 255) / 256;
        gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
        hipLaunchKernelGGL(heldout_snapshot_kernel, dim3((unsigned)gx, (unsigned)m.n_segs), dim3(256), 0, st, (const HeldoutSeg*)m.segs,
                           (const HeldoutState*)m.state);
        check_launch("heldout_snapshot");
    }
}

// what skf_iterate runs after every iterate_fit of a monitored plan, on the same stream
static void heldout_step(skf_plan* p, hipStream_t st) { heldout_eval(p, true, st); }

static HeldoutState heldout_read_state(const skf_plan* p, hipStream_t st) {
    HeldoutState s;
    SKF_HIP(hipMemcpyAsync(&s, p->mon.state, sizeof s, hipMemcpyDeviceToHost, st));
    SKF_HIP(hipStreamSynchronize(st));
    return s;
}

extern "C" {

int skf_plan_heldout_workspace_bytes(const skf_plan* p, int32_t n_lists, const skf_heldout_desc* descs, int64_t capacity_iters,
                                     size_t* bytes) {
    return guarded([&] {
        if (!bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        heldout_check_plan(p, n_lists, descs, capacity_iters);
        *bytes = heldout_layout(p, n_lists, descs, capacity_iters).total;
    });
}

int skf_plan_set_heldout(skf_plan* p, int32_t n_lists, const skf_heldout_desc* descs, int32_t patience, double min_delta,
                         int64_t capacity_iters, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] {
        if (!p) SKF_FAIL(SKF_E_INVALID, "null plan");
        p->mon = HeldoutMonitor();                         // whatever happens below, the previous monitor is gone
        if (!p->bound) SKF_FAIL(SKF_E_STATE, "workspace not bound");
        if (n_lists == 0) return;                          // detach
        heldout_check_plan(p, n_lists, descs, capacity_iters);
        if (patience < 0) SKF_FAIL(SKF_E_INVALID, "held-out lists: patience %d is negative", patience);
        if (min_delta != min_delta || min_delta < 0.0) SKF_FAIL(SKF_E_INVALID, "held-out lists: min_delta must be >= 0");
        const HeldoutLayout L = heldout_layout(p, n_lists, descs, capacity_iters);
        if (!workspace || ((uintptr_t)workspace & 255) != 0) SKF_FAIL(SKF_E_INVALID, "held-out lists: the workspace must be 256-byte aligned");
        if (workspace_bytes < L.total)
            SKF_FAIL(SKF_E_INVALID, "held-out lists: workspace %zu B < required %zu B (skf_plan_heldout_workspace_bytes)", workspace_bytes, L.total);
        hipStream_t st = as_stream(stream);
        char* base = (char*)workspace;
        HeldoutMonitor m;
        m.state = (HeldoutState*)(base + L.state);
        // the lists, on the device, before anything gathers through them
        for (int l = 0; l < n_lists; ++l) {
            const RelState& r = p->rels[descs[l].rel];
            const int64_t ni = p->types[r.row].n, nj = p->types[r.col].n;
            const int64_t n = descs[l].n;
            const int bad = device_flag(&m.state->bad, st, [&] {
                if (p->f64)
                    hipLaunchKernelGGL((heldout_check_kernel<double>), dim3(elem_grid(n)), dim3(256), 0, st, (const int*)descs[l].rows,
                                       (const int*)descs[l].cols, (const double*)descs[l].values, n, ni, nj, &m.state->bad);
                else
                    hipLaunchKernelGGL((heldout_check_kernel<float>), dim3(elem_grid(n)), dim3(256), 0, st, (const int*)descs[l].rows,
                                       (const int*)descs[l].cols, (const float*)descs[l].values, n, ni, nj, &m.state->bad);
                check_launch("heldout_check");
            });
            if (bad)
                SKF_FAIL(SKF_E_INVALID, "held-out list %d (relation %d): a row outside 0 .. %lld, a column outside 0 .. %lld, rows that decrease or a value that is not finite",
                         l, descs[l].rel, (long long)ni - 1, (long long)nj - 1);
        }
        m.patience = patience;
        m.min_delta = min_delta;
        m.capacity = capacity_iters;
        m.offs = (int64_t*)(base + L.offs);
        m.cur = (double*)(base + L.cur);
        m.segs = (HeldoutSeg*)(base + L.segs);
        m.partials = (double*)(base + L.partials);
        m.history = (double*)(base + L.history);
        m.host_offs.push_back(0);
        for (int l = 0; l < n_lists; ++l) {
            HeldoutList hl;
            hl.rel = descs[l].rel; hl.n = descs[l].n;
            hl.rows = (const int*)descs[l].rows; hl.cols = (const int*)descs[l].cols; hl.vals = descs[l].values;
            hl.blocks = L.blocks[l];
            hl.H = base + L.H[l];
            hl.part = L.part_bytes[l] ? base + L.part[l] : nullptr;
            hl.part_bytes = L.part_bytes[l];
            m.lists.push_back(hl);
            m.host_offs.push_back(m.host_offs.back() + hl.blocks);
        }
        for (size_t i = 0; i < p->types.size(); ++i) {
            const TypeState& t = p->types[i];
            m.snap_g.push_back(base + L.snap_g[i]);
            const int64_t words = (int64_t)((size_t)t.n * t.c * p->esz / 4);
            m.host_segs.push_back(HeldoutSeg{(const unsigned*)t.G.ptr, (unsigned*)m.snap_g.back(), words});
            m.max_words = std::max(m.max_words, words);
        }
        for (size_t k = 0; k < p->rels.size(); ++k) {
            const RelState& r = p->rels[k];
            m.snap_s.push_back(base + L.snap_s[k]);
            const int64_t words = (int64_t)p->types[r.row].c * p->types[r.col].c * 2;
            m.host_segs.push_back(HeldoutSeg{(const unsigned*)r.S.ptr, (unsigned*)m.snap_s.back(), words});
            m.max_words = std::max(m.max_words, words);
        }
        m.n_segs = (int)m.host_segs.size();
        HeldoutState init;
        memset(&init, 0, sizeof init);
        init.best = INFINITY;
        SKF_HIP(hipMemcpyAsync(m.state, &init, sizeof init, hipMemcpyHostToDevice, st));
        SKF_HIP(hipMemcpyAsync(m.offs, m.host_offs.data(), m.host_offs.size() * 8, hipMemcpyHostToDevice, st));
        SKF_HIP(hipMemcpyAsync(m.segs, m.host_segs.data(), m.host_segs.size() * sizeof(HeldoutSeg), hipMemcpyHostToDevice, st));
        SKF_HIP(hipStreamSynchronize(st));                 // (the uploads read host memory of this frame)
        p->mon = std::move(m);
        if (p->graph_exec) {                               // a captured iteration knows nothing of the monitor
            (void)hipGraphExecDestroy(p->graph_exec);
            p->graph_exec = nullptr;
        }
    });
}

int skf_plan_heldout_sqerr(skf_plan* p, double* out, void* stream) {
    return guarded([&] {
        heldout_check_ready(p, "skf_plan_heldout_sqerr");
        if (!out) SKF_FAIL(SKF_E_INVALID, "skf_plan_heldout_sqerr: null pointer");
        for (size_t i = 0; i < p->types.size(); ++i)
            if (!p->types[i].set) SKF_FAIL(SKF_E_STATE, "factor of object type %zu not set", i);
        for (const HeldoutList& hl : p->mon.lists)
            if (p->first_iter && !p->rels[hl.rel].s_set)
                SKF_FAIL(SKF_E_STATE, "backbone of relation %d neither set nor computed yet", hl.rel);
        hipStream_t st = as_stream(stream);
        heldout_eval(p, false, st);
        SKF_HIP(hipMemcpyAsync(out, p->mon.cur, p->mon.lists.size() * 8, hipMemcpyDeviceToDevice, st));
    });
}

int skf_plan_get_heldout_product(const skf_plan* p, int32_t list, void* H, int64_t ld, void* stream) {
    return guarded([&] {
        heldout_check_ready(p, "skf_plan_get_heldout_product");
        if (list < 0 || list >= (int)p->mon.lists.size() || !H) SKF_FAIL(SKF_E_INVALID, "skf_plan_get_heldout_product: bad list index / pointer");
        const HeldoutList& hl = p->mon.lists[list];
        const RelState& r = p->rels[hl.rel];
        const int cj = p->types[r.col].c;
        if (ld < cj) SKF_FAIL(SKF_E_INVALID, "ld too small");
        copy2d(H, ld, hl.H, cj, p->types[r.row].n, cj, p->esz, as_stream(stream));
    });
}

int skf_plan_get_monitor(const skf_plan* p, int64_t* seen, int64_t* best_iter, int64_t* stop_iter, int32_t* stopped, double* best,
                         double* history_host, int64_t capacity, void* stream) {
    return guarded([&] {
        heldout_check_ready(p, "skf_plan_get_monitor");
        if (capacity < 0 || (capacity > 0 && !history_host)) SKF_FAIL(SKF_E_INVALID, "skf_plan_get_monitor: bad history buffer");
        hipStream_t st = as_stream(stream);
        const HeldoutState s = heldout_read_state(p, st);
        if (seen) *seen = s.seen;
        if (best_iter) *best_iter = s.best_iter;
        if (stop_iter) *stop_iter = s.stop_iter;
        if (stopped) *stopped = s.stopped;
        if (best) *best = s.best;
        const int64_t rows = std::min(std::min(s.seen, p->mon.capacity), capacity);
        if (rows > 0) {
            SKF_HIP(hipMemcpyAsync(history_host, p->mon.history, (size_t)rows * p->mon.lists.size() * 8, hipMemcpyDeviceToHost, st));
            SKF_HIP(hipStreamSynchronize(st));
        }
    });
}

int skf_get_best_factor(const skf_plan* p, int32_t type, void* G, int64_t ld, void* stream) {
    return guarded([&] {
        heldout_check_ready(p, "skf_get_best_factor");
        if (type < 0 || type >= (int)p->types.size() || !G) SKF_FAIL(SKF_E_INVALID, "bad type index / pointer");
        const TypeState& t = p->types[type];
        if (ld < t.c) SKF_FAIL(SKF_E_INVALID, "ld %lld < rank %d", (long long)ld, t.c);
        hipStream_t st = as_stream(stream);
        if (heldout_read_state(p, st).best_iter == 0) SKF_FAIL(SKF_E_STATE, "skf_get_best_factor: no judged iteration has a best model yet");
        copy2d(G, ld, p->mon.snap_g[type], t.c, t.n, t.c, p->esz, st);
    });
}

int skf_get_best_backbone(const skf_plan* p, int32_t rel, void* S, int64_t ld, void* stream) {
    return guarded([&] {
        heldout_check_ready(p, "skf_get_best_backbone");
        if (rel < 0 || rel >= (int)p->rels.size() || !S) SKF_FAIL(SKF_E_INVALID, "bad relation index / pointer");
        const RelState& r = p->rels[rel];
        const int ci = p->types[r.row].c, cj = p->types[r.col].c;
        if (ld < cj) SKF_FAIL(SKF_E_INVALID, "ld too small");
        hipStream_t st = as_stream(stream);
        if (heldout_read_state(p, st).best_iter == 0) SKF_FAIL(SKF_E_STATE, "skf_get_best_backbone: no judged iteration has a best model yet");
        if (p->f64) {
            copy2d(S, ld, p->mon.snap_s[rel], cj, ci, cj, 8, st);
        } else {                                           // (as skf_get_backbone: the f64 backbone in the master type)
            hipLaunchKernelGGL((cast_kernel<float, double>), dim3(elem_grid((int64_t)ci * cj)), dim3(256), 0, st, (float*)S, ld,
                               (const double*)p->mon.snap_s[rel], (int64_t)cj, (int64_t)ci, (int64_t)cj);
            check_launch("cast");
        }
    });
}

}  // extern "C"
