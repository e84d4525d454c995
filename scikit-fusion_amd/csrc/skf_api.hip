// skf_api.hip -- the C ABI (include/skfusion_hip.h): the includes of the one translation unit, its error / launch counters
// and small helpers, and the entry points.  Kernels: skf_kernels.h; the plan and its launch primitives: skf_plan.inc; plan
// creation: skf_create.inc; the steps and schedules of the DFMF / DFMC / fold-in iteration: skf_steps.inc, skf_stages.inc,
// skf_schedule.inc, skf_dist.inc; what a bind builds: skf_bind.inc; the relation objective: skf_objective.inc; the
// pseudo-inverse: skf_pinv.h / .inc; the completion operators (skf_complete_*): kernels skf_complete.h, host side and entry
// points skf_complete.inc; the column-mean initialisers on the device (skf_plan_relation_norms,
// skf_plan_init_column_means): kernels skf_init.h, host side and entry points skf_init.inc.
//
// One iteration (reference _dfmf.py:228-296, 2-GEMM form of SURVEY.md 7.0; everything reads the
// OLD factors, G is replaced at the very end):
//   Gram_i = G_i^T G_i                    split-K MFMA GEMM + fixed-order reduce   (:228-231)
//   K_i    = pinv(Gram_i)                 Jacobi eigen kernel, one workgroup/type  (:232)
//   P_r = R_r G_j ; Q_r = R_r^T G_i       the two big contractions (only reads of R)
//   S_r = K_i (G_i^T P_r) K_j             (:236-239)
//   [DFMC] R_r[mask] = (G_i S_r G_j^T)[mask], P_r recomputed               (_dfmc.py:319-325)
//   E_i += (P_r S_r^T)+ + G_i B-  ; D_i += (P_r S_r^T)- + G_i B+ ,  B = S Gram_j S^T  (:254-281)
//   E_j += (Q_r S_r)+   + G_j D-  ; D_j += (Q_r S_r)-   + G_j D+ ,  D = S^T Gram_i S
//   D_i += Theta+ G_i ; E_i += Theta- G_i                                   (:284-292)
//   G_i <- G_i * sqrt(E_i / max(D_i, eps))                                  (:294-296)
#include "skf_kernels.h"
#include "skf_known.h"
#include "skf_pinv.h"
#include "skf_small.h"
#include "skf_complete.h"
#include "skf_init.h"
#include "skf_heldout.h"
// the product build compiles the GEMM-class kernel templates in units of their own, side by side with this file
// (tools/gen_inst_units.py, __graft_entry__.build); a build of this file alone (emulator, probes) instantiates them here
#ifdef SKF_SPLIT_BUILD
#include "skf_inst_decl.h"
#endif

#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/skfusion_hip.h"

struct skf_comm;

namespace skf {

static thread_local std::string g_err;

struct Error {
    int code;
    std::string msg;
};

#define SKF_FAIL(code_, ...)                                  \
    do {                                                      \
        char buf_[512];                                       \
        snprintf(buf_, sizeof buf_, __VA_ARGS__);             \
        throw Error{(code_), std::string(buf_)};              \
    } while (0)

#define SKF_HIP(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) SKF_FAIL(SKF_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// the ONE place the library reads its environment (test / A-B switches: Switches::read and plan creation; SKF_RCCL_PATH)
static const char* env_str(const char* name) { return getenv(name); }
static int env_int(const char* name, int unset) {
    const char* v = env_str(name);
    return v ? atoi(v) : unset;
}

static thread_local int64_t g_split_clamps = 0;  // split-K launches whose slice count the scratch could not hold (skf_split_clamps)
static thread_local int64_t g_launches = 0;      // kernel launches this thread has issued through the library (skf_launch_count)

static inline void check_launch(const char* what) {
    ++g_launches;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) SKF_FAIL(SKF_E_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
}

template <class F>
static int guarded(F&& f) {
    try {
        f();
        return SKF_OK;
    } catch (const Error& e) {
        g_err = e.msg;
        return e.code;
    } catch (const std::exception& e) {
        g_err = e.what();
        return SKF_E_INVALID;
    }
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// SKF_OPT_OWNED_ROWS: rows per rank of a type of n objects over `world` ranks (include/skfusion_hip.h, skf_owned_rows):
// boundaries at multiples of the 256-row contraction tile for large types, of 64 for SKF_BF16 (the K padding of Q = R^T G_i)
static inline int64_t owned_chunk(int dtype, int64_t n, int world) {
    const int64_t per = (n + world - 1) / world;
    const int64_t a = per >= 1024 ? 256 : (dtype == 2 /* SKF_BF16 */ ? 64 : 1);
    return (per + a - 1) / a * a;
}
static inline int elem_grid(int64_t total) {
    int64_t b = (total + 255) / 256;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;           // grid-stride the rest (256 CUs x 8 blocks)
    return (int)b;
}
// one wave per row, four rows per workgroup of 256 threads; the rows past 2048 workgroups by grid stride
static inline int wave_grid(int64_t rows) {
    int64_t b = (rows + 3) / 4;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (int)b;
}

#include "skf_gemm_launch.inc"

#include "skf_plan.inc"

#include "skf_pinv.inc"

#include "skf_steps.inc"

#include "skf_stages.inc"

#include "skf_dist.inc"

#include "skf_schedule.inc"

#include "skf_bind.inc"

#include "skf_objective.inc"

#include "skf_complete.inc"

#include "skf_init.inc"

#include "skf_heldout.inc"

}  // namespace skf

using namespace skf;

#include "skf_create.inc"

extern "C" {

const char* skf_last_error(void) { return g_err.c_str(); }
const char* skf_version(void) { return "skfusion_hip 0.1 (gfx950)"; }

int skf_plan_create(int32_t n_types, const skf_type_desc* types, int32_t n_relations,
                    const skf_relation_desc* relations, int32_t n_thetas, const skf_theta_desc* thetas,
                    const skf_options* opt, skf_plan** out) {
    return guarded([&] {
        if (!out || !types || !opt || n_types <= 0) SKF_FAIL(SKF_E_INVALID, "null argument / no object types");
        if (n_relations < 0 || n_thetas < 0 || (n_relations > 0 && !relations) || (n_thetas > 0 && !thetas))
            SKF_FAIL(SKF_E_INVALID, "bad relation / constraint arrays");
        if (opt->dtype != SKF_F64 && opt->dtype != SKF_F32 && opt->dtype != SKF_BF16)
            SKF_FAIL(SKF_E_INVALID, "unknown dtype %d", opt->dtype);
        if (opt->dtype == SKF_BF16 && opt->engine != SKF_ENGINE_MFMA)
            SKF_FAIL(SKF_E_INVALID, "SKF_BF16 needs the MFMA engine");
        if (opt->variant < SKF_DFMF || opt->variant > SKF_TRANSFORM) SKF_FAIL(SKF_E_INVALID, "bad variant");
        if (opt->engine != SKF_ENGINE_MFMA && opt->engine != SKF_ENGINE_VALU) SKF_FAIL(SKF_E_INVALID, "bad engine");
        skf_plan* p = new skf_plan();
        struct Guard { skf_plan* p; ~Guard() { delete p; } } guard{p};
        plan_describe_types(p, n_types, types, opt);
        plan_describe_relations(p, n_types, n_relations, relations);
        plan_decide_lists(p, relations);
        plan_describe_constraints(p, n_types, n_thetas, thetas);
        plan_layout(p);
        guard.p = nullptr;
        *out = p;
    });
}

int skf_plan_destroy(skf_plan* plan) {
    delete plan;
    return SKF_OK;
}

int skf_plan_set_known_entries(skf_plan* plan, int32_t rel, const int64_t* indptr, const int32_t* indices, const void* values) {
    return guarded([&] {
        if (!plan) SKF_FAIL(SKF_E_INVALID, "null argument");
        if (plan->ws_base) SKF_FAIL(SKF_E_STATE, "skf_plan_set_known_entries after skf_plan_bind_workspace");
        if (rel < 0 || rel >= (int)plan->rels.size()) SKF_FAIL(SKF_E_INVALID, "relation %d out of range", rel);
        RelState& r = plan->rels[rel];
        if (!r.kn_csr && !r.sp0 && !r.fold)
            SKF_FAIL(SKF_E_INVALID, "relation %d is flagged neither SKF_REL_KNOWN_CSR, SKF_REL_SPARSE_CSR nor SKF_REL_FOLD_CSR", rel);
        if (r.absent) SKF_FAIL(SKF_E_INVALID, "relation %d is SKF_REL_ABSENT here: it takes no lists", rel);
        if (!indptr || (r.kn_cap > 0 && (!indices || !values))) SKF_FAIL(SKF_E_INVALID, "relation %d: null CSR array", rel);
        r.csr_ptr = indptr;
        r.csr_idx = (const int*)indices;
        r.csr_val = values;
    });
}

int skf_plan_set_relation_fill(skf_plan* plan, int32_t rel, const void* row_fill, const void* col_fill, void* stream) {
    return guarded([&] {
        (void)stream;       // (the vectors are read by skf_plan_bind_workspace on ITS stream, like the lists)
        if (!plan) SKF_FAIL(SKF_E_INVALID, "null argument");
        if (plan->ws_base) SKF_FAIL(SKF_E_STATE, "skf_plan_set_relation_fill after skf_plan_bind_workspace");
        if (rel < 0 || rel >= (int)plan->rels.size()) SKF_FAIL(SKF_E_INVALID, "relation %d out of range", rel);
        RelState& r = plan->rels[rel];
        if (!r.fill) SKF_FAIL(SKF_E_INVALID, "relation %d is not flagged SKF_REL_FILL_RANK1", rel);
        if (!row_fill || !col_fill) SKF_FAIL(SKF_E_INVALID, "relation %d: null fill vector", rel);
        r.fill_row = row_fill;
        r.fill_col = col_fill;
    });
}

int skf_plan_set_constraint_entries(skf_plan* plan, int32_t theta, const int64_t* indptr, const int32_t* indices, const void* values) {
    return guarded([&] {
        if (!plan) SKF_FAIL(SKF_E_INVALID, "null argument");
        if (plan->ws_base) SKF_FAIL(SKF_E_STATE, "skf_plan_set_constraint_entries after skf_plan_bind_workspace");
        if (theta < 0 || theta >= (int)plan->thetas.size()) SKF_FAIL(SKF_E_INVALID, "constraint %d out of range", theta);
        ThetaState& th = plan->thetas[theta];
        if (!th.entries) SKF_FAIL(SKF_E_INVALID, "constraint %d has a dense form (skf_theta_desc.data)", theta);
        if (!indptr || (th.nnz_cap > 0 && (!indices || !values))) SKF_FAIL(SKF_E_INVALID, "constraint %d: null CSR array", theta);
        th.csr_ptr = indptr;
        th.csr_idx = (const int*)indices;
        th.csr_val = values;
    });
}

int skf_plan_workspace_bytes(const skf_plan* plan, size_t* bytes) {
    return guarded([&] {
        if (!plan || !bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        *bytes = plan->ws_bytes;
    });
}

int skf_plan_bind_workspace(skf_plan* p, void* ws, size_t bytes, void* stream) {
    return guarded([&] {
        if (!p || !ws) SKF_FAIL(SKF_E_INVALID, "null argument");
        if (bytes < p->ws_bytes) SKF_FAIL(SKF_E_WORKSPACE, "workspace %zu B < required %zu B", bytes, p->ws_bytes);
        if (((uintptr_t)ws & 255) != 0) SKF_FAIL(SKF_E_WORKSPACE, "workspace must be 256-byte aligned");
        for (Slot* s : p->slots) s->ptr = (char*)ws + s->off;
        p->ws_base = ws;
        p->sw = Switches::read();          // the only place a plan looks at the environment
        hipStream_t st = as_stream(stream);
        bind_relation_lists(p, st);
        bind_bf16_copies(p, st);
        bind_theta_csr(p, st);
        bind_theta_halves(p, st);
        bind_pinv_tables(p, st);
        bind_small_tables(p, st);
        bind_owned_clears(p, st);
        bind_streams(p);
        if (p->graph_exec) {
            (void)hipGraphExecDestroy(p->graph_exec);
            p->graph_exec = nullptr;
        }
        p->graph_failed = false;
        p->mon = HeldoutMonitor();           // (a monitor lives in a workspace of its own and belongs to the binding it was attached to)
        p->bound = true;
        p->prepared = false;
        p->first_iter = true;
        p->kn_first = true;
    });
}

static void check_bound(const skf_plan* p) {
    if (!p) SKF_FAIL(SKF_E_INVALID, "null plan");
    if (!p->bound) SKF_FAIL(SKF_E_STATE, "workspace not bound");
}

int skf_set_factor(skf_plan* p, int32_t type, const void* G, int64_t ld, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (type < 0 || type >= (int)p->types.size() || !G) SKF_FAIL(SKF_E_INVALID, "bad type index / pointer");
        TypeState& t = p->types[type];
        if (ld < t.c) SKF_FAIL(SKF_E_INVALID, "ld %lld < rank %d", (long long)ld, t.c);
        copy2d(t.G.ptr, t.c, G, ld, t.n, t.c, p->esz, as_stream(stream));
        refresh_gt(p, t, as_stream(stream));
        t.set = true;
        p->prepared = false;
    });
}

int skf_get_factor(const skf_plan* p, int32_t type, void* G, int64_t ld, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (type < 0 || type >= (int)p->types.size() || !G) SKF_FAIL(SKF_E_INVALID, "bad type index / pointer");
        const TypeState& t = p->types[type];
        if (ld < t.c) SKF_FAIL(SKF_E_INVALID, "ld %lld < rank %d", (long long)ld, t.c);
        copy2d(G, ld, t.G.ptr, t.c, t.n, t.c, p->esz, as_stream(stream));
    });
}

int skf_set_backbone(skf_plan* p, int32_t rel, const void* S, int64_t ld, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (rel < 0 || rel >= (int)p->rels.size() || !S) SKF_FAIL(SKF_E_INVALID, "bad relation index / pointer");
        RelState& r = p->rels[rel];
        const int ci = p->types[r.row].c, cj = p->types[r.col].c;
        if (ld < cj) SKF_FAIL(SKF_E_INVALID, "ld too small");
        if (p->f64) {
            copy2d(r.S.ptr, cj, S, ld, ci, cj, 8, as_stream(stream));
        } else {
            hipLaunchKernelGGL((cast_kernel<double, float>), dim3(elem_grid((int64_t)ci * cj)), dim3(256), 0,
                               as_stream(stream), (double*)r.S.ptr, (int64_t)cj, (const float*)S, ld, (int64_t)ci,
                               (int64_t)cj);
            check_launch("cast");
        }
        r.s_set = true;
        p->prepared = false;
    });
}

int skf_get_backbone(const skf_plan* p, int32_t rel, void* S, int64_t ld, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (rel < 0 || rel >= (int)p->rels.size() || !S) SKF_FAIL(SKF_E_INVALID, "bad relation index / pointer");
        const RelState& r = p->rels[rel];
        const int ci = p->types[r.row].c, cj = p->types[r.col].c;
        if (ld < cj) SKF_FAIL(SKF_E_INVALID, "ld too small");
        if (p->f64) {
            copy2d(S, ld, r.S.ptr, cj, ci, cj, 8, as_stream(stream));
        } else {
            hipLaunchKernelGGL((cast_kernel<float, double>), dim3(elem_grid((int64_t)ci * cj)), dim3(256), 0,
                               as_stream(stream), (float*)S, ld, (const double*)r.S.ptr, (int64_t)cj, (int64_t)ci,
                               (int64_t)cj);
            check_launch("cast");
        }
    });
}

int skf_iterate(skf_plan* p, int32_t n_iters, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (p->sliced) SKF_FAIL(SKF_E_STATE, "a plan with row blocks iterates through skf_stage + the exchanges");
        if (n_iters < 0) SKF_FAIL(SKF_E_INVALID, "n_iters < 0");
        for (size_t i = 0; i < p->types.size(); ++i)
            if (!p->types[i].set) SKF_FAIL(SKF_E_STATE, "factor of object type %zu not set", i);
        hipStream_t st = as_stream(stream);
        if (p->variant == SKF_TRANSFORM) {
            for (size_t r = 0; r < p->rels.size(); ++r)
                if (!p->rels[r].s_set) SKF_FAIL(SKF_E_STATE, "backbone of relation %zu not set", r);
            if (!p->prepared) prepare_transform(p, st);
            for (int it = 0; it < n_iters; ++it) iterate_transform(p, st);
        } else {
            int it = 0;
            // a monitored plan (skf_plan_set_heldout): the held-out lists are scored and judged after every iteration, on
            // the same stream; never the hipGraph path
            if (monitored(p))
                for (; it < n_iters; ++it) {
                    iterate_fit(p, st);
                    heldout_step(p, st);
                }
            // The iteration is ~50-80 launches; for small graphs (launch-latency regime) the
            // remaining iterations replay ONE captured hipGraph.  Capture needs a real stream
            // (not the legacy default stream) and is skipped while profiling events are recorded.
            if (use_graph(p, st, n_iters)) {
                if (p->first_iter || !p->graph_exec || p->graph_stream != st) {
                    iterate_fit(p, st);               // eager: first-iteration work, attributes
                    ++it;
                    capture_iteration(p, st);
                }
                if (p->graph_exec)
                    for (; it < n_iters; ++it) SKF_HIP(hipGraphLaunch(p->graph_exec, st));
            }
            for (; it < n_iters; ++it) iterate_fit(p, st);
        }
    });
}

int skf_iterate_batch(skf_plan* const* plans, int32_t n_plans, int32_t n_iters, void* stream) {
    return guarded([&] {
        if (!plans || n_plans < 1 || n_plans > SKF_MAX_BATCH) SKF_FAIL(SKF_E_INVALID, "1 .. %d plans", SKF_MAX_BATCH);
        if (n_iters < 0) SKF_FAIL(SKF_E_INVALID, "n_iters < 0");
        skf_plan* p0 = plans[0];
        if (p0 && p0->variant == SKF_TRANSFORM) {
            // fold-ins of one graph into the models of several restarts (reference dfmf.py:191-199): same new relations, the
            // frozen factors / backbones of each restart in its own plan; one launch per iteration serves all of them
            for (int k = 0; k < n_plans; ++k) {
                skf_plan* p = plans[k];
                check_bound(p);
                for (const RelState& r : p->rels)
                    if (r.fold_known) SKF_FAIL(SKF_E_INVALID, "plan %d holds a SKF_REL_FOLD_KNOWN relation: such fold-ins do not batch", k);
                if (!fold_fused(p) || p->dtype != p0->dtype || p->types.size() != p0->types.size() || p->rels.size() != p0->rels.size() ||
                    p->target != p0->target)
                    SKF_FAIL(SKF_E_STATE, "plan %d does not batch with plan 0 (fold-in without constraints on the target, same graph and engine required)", k);
                for (size_t i = 0; i < p->types.size(); ++i) {
                    if (p->types[i].n != p0->types[i].n || p->types[i].c != p0->types[i].c)
                        SKF_FAIL(SKF_E_STATE, "plan %d: object type %zu differs from plan 0", k, i);
                    if (!p->types[i].set) SKF_FAIL(SKF_E_STATE, "plan %d: factor of object type %zu not set", k, i);
                }
                for (size_t r = 0; r < p->rels.size(); ++r) {
                    if (p->rels[r].row != p0->rels[r].row || p->rels[r].col != p0->rels[r].col)
                        SKF_FAIL(SKF_E_STATE, "plan %d: relation %zu differs from plan 0", k, r);
                    if (!p->rels[r].s_set) SKF_FAIL(SKF_E_STATE, "plan %d: backbone of relation %zu not set", k, r);
                }
                for (int q = 0; q < k; ++q)
                    if (plans[q] == p) SKF_FAIL(SKF_E_INVALID, "plan %d listed twice", k);
            }
            hipStream_t st = as_stream(stream);
            for (int k = 0; k < n_plans; ++k)
                if (!plans[k]->prepared) prepare_transform(plans[k], st);
            fold_steps(plans, n_plans, n_iters, st);
            return;
        }
        for (int k = 0; k < n_plans; ++k) {
            skf_plan* p = plans[k];
            check_bound(p);
            if (monitored(p)) SKF_FAIL(SKF_E_STATE, "plan %d scores held-out lists (skf_plan_set_heldout): it does not batch", k);
            for (size_t i = 0; i < p->types.size(); ++i)
                if (!p->types[i].set) SKF_FAIL(SKF_E_STATE, "plan %d: factor of object type %zu not set", k, i);
            // one launch serves every plan (plan 0's grid, LDS and job tables): the small-graph schedule, the same engine and
            // the same graph -- object counts, ranks, relation and constraint structure compared field by field
            bool same = p->small_fused && p->f64 == p0->f64 && p->variant == p0->variant && p->engine == p0->engine &&
                        p->types.size() == p0->types.size() && p->rels.size() == p0->rels.size() &&
                        p->thetas.size() == p0->thetas.size() && p->sm_j1.size() == p0->sm_j1.size() &&
                        p->sm_j3.size() == p0->sm_j3.size();
            for (size_t i = 0; same && i < p->types.size(); ++i)
                same = p->types[i].n == p0->types[i].n && p->types[i].c == p0->types[i].c;
            for (size_t r = 0; same && r < p->rels.size(); ++r)
                same = p->rels[r].row == p0->rels[r].row && p->rels[r].col == p0->rels[r].col;
            for (size_t t = 0; same && t < p->thetas.size(); ++t)
                same = p->thetas[t].type == p0->thetas[t].type && p->thetas[t].sparse == p0->thetas[t].sparse;
            auto same_job = [](const SmJob& a, const SmJob& b) {
                return a.kind == b.kind && a.idx == b.idx && a.r0 == b.r0 && a.nr == b.nr && a.part == b.part && a.k0 == b.k0 && a.nk == b.nk;
            };
            for (size_t j = 0; same && j < p->sm_j1.size(); ++j) same = same_job(p->sm_j1[j], p0->sm_j1[j]);
            for (size_t j = 0; same && j < p->sm_j3.size(); ++j) same = same_job(p->sm_j3[j], p0->sm_j3[j]);
            if (!same)
                SKF_FAIL(SKF_E_STATE, "plan %d does not batch with plan 0 (small-graph schedule, same graph and engine required)", k);
            for (int q = 0; q < k; ++q)
                if (plans[q] == p) SKF_FAIL(SKF_E_INVALID, "plan %d listed twice", k);
        }
        hipStream_t st = as_stream(stream);
        std::vector<const void*> tabs((size_t)n_plans);
        for (int k = 0; k < n_plans; ++k) tabs[(size_t)k] = plans[k]->sm_tables.ptr;
        if (tabs != p0->sm_batch_host) {                  // (the table of tables lives in plan 0's workspace; [0] stays plan 0's own)
            p0->sm_batch_host = tabs;
            SKF_HIP(hipMemcpyAsync(p0->sm_batch.ptr, p0->sm_batch_host.data(), tabs.size() * sizeof(void*), hipMemcpyHostToDevice, st));
        }
        for (int it = 0; it < n_iters; ++it) {
            if (p0->f64) iterate_small_fused_t<double>(p0, st, (unsigned)n_plans);
            else iterate_small_fused_t<float>(p0, st, (unsigned)n_plans);
        }
        for (int k = 0; k < n_plans; ++k) plans[k]->first_iter = false;
    });
}

int skf_plan_batchable(const skf_plan* p, int32_t* yes) {
    return guarded([&] {
        check_bound(p);
        if (!yes) SKF_FAIL(SKF_E_INVALID, "null pointer");
        *yes = ((p->small_fused || fold_fused(p)) && !monitored(p)) ? 1 : 0;
    });
}

int skf_small_graph_limits(int32_t* max_rank, int64_t* max_objects, int32_t* max_types, int32_t* max_relations,
                           int32_t* max_constraints, int32_t* constraint_nnz_divisor) {
    return guarded([&] {
        if (max_rank) *max_rank = SMALLC;
        if (max_objects) *max_objects = SM_MAX_OBJECTS;
        if (max_types) *max_types = SM_MAXT;
        if (max_relations) *max_relations = SM_MAXR;
        if (max_constraints) *max_constraints = SM_MAXTH;
        if (constraint_nnz_divisor) *constraint_nnz_divisor = SKF_THETA_SPARSE_DIV;
    });
}

int skf_plan_set_graph(skf_plan* p, int32_t enable) {
    return guarded([&] {
        if (!p) SKF_FAIL(SKF_E_INVALID, "null plan");
        p->graph_on = enable != 0;
    });
}

int skf_accumulate(skf_plan* p, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (p->variant == SKF_TRANSFORM) SKF_FAIL(SKF_E_INVALID, "skf_accumulate: SKF_DFMF / SKF_DFMC plans only");
        if (p->owned) SKF_FAIL(SKF_E_STATE, "a plan with owned rows (SKF_OPT_OWNED_ROWS) iterates through skf_iterate_dist");
        for (size_t i = 0; i < p->types.size(); ++i)
            if (!p->types[i].set) SKF_FAIL(SKF_E_STATE, "factor of object type %zu not set", i);
        accumulate_fit(p, as_stream(stream));
    });
}

int skf_apply_update(skf_plan* p, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (p->variant == SKF_TRANSFORM) SKF_FAIL(SKF_E_INVALID, "skf_apply_update: SKF_DFMF / SKF_DFMC plans only");
        apply_update(p, as_stream(stream));
    });
}

int skf_stage(skf_plan* p, int32_t stage, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (p->variant == SKF_TRANSFORM) SKF_FAIL(SKF_E_INVALID, "skf_stage: SKF_DFMF / SKF_DFMC plans only");
        if (p->owned) SKF_FAIL(SKF_E_STATE, "a plan with owned rows (SKF_OPT_OWNED_ROWS) iterates through skf_iterate_dist");
        for (size_t i = 0; i < p->types.size(); ++i)
            if (!p->types[i].set) SKF_FAIL(SKF_E_STATE, "factor of object type %zu not set", i);
        hipStream_t st = as_stream(stream);
        switch (stage) {
            case SKF_STAGE_CONTRACT: stage_contract(p, st); break;
            case SKF_STAGE_BACKBONE: stage_backbone(p, st); break;
            case SKF_STAGE_ACCUMULATE: stage_accumulate(p, st); break;
            case SKF_STAGE_UPDATE: apply_update(p, st); break;
            default: SKF_FAIL(SKF_E_INVALID, "unknown stage %d", stage);
        }
    });
}

int skf_exchange_range(const skf_plan* p, int32_t which, size_t* offset, size_t* bytes, int32_t* dtype) {
    return guarded([&] {
        if (!p || !offset || !bytes || !dtype) SKF_FAIL(SKF_E_INVALID, "null argument");
        *dtype = p->mt;
        switch (which) {
            case SKF_X_W: *offset = p->xw_off; *bytes = p->xw_bytes; *dtype = SKF_F64; break;
            case SKF_X_Q: *offset = p->xq_off; *bytes = p->xq_bytes; break;
            case SKF_X_QM: *offset = p->xqm_off; *bytes = p->xqm_bytes; break;
            case SKF_X_ED: *offset = p->acc_off; *bytes = p->acc_bytes; break;
            default: SKF_FAIL(SKF_E_INVALID, "unknown exchange range %d", which);
        }
    });
}

int skf_accumulator_range(const skf_plan* p, size_t* offset, size_t* bytes) {
    return guarded([&] {
        if (!p || !offset || !bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        *offset = p->acc_off;
        *bytes = p->acc_bytes;
    });
}

int skf_comm_unique_id(void* id128) {
    return guarded([&] {
        if (!id128) SKF_FAIL(SKF_E_INVALID, "null argument");
        NcclUniqueId id;
        const int rc = rccl().get_unique_id(&id);
        if (rc != 0) SKF_FAIL(SKF_E_HIP, "ncclGetUniqueId failed (%d)", rc);
        memcpy(id128, &id, sizeof id);
    });
}

int skf_comm_create(const void* id128, int32_t rank, int32_t world, skf_comm** out) {
    return guarded([&] {
        if (!out || world < 1 || rank < 0 || rank >= world) SKF_FAIL(SKF_E_INVALID, "bad rank / world / pointer");
        skf_comm* c = new skf_comm();
        c->rank = rank; c->world = world;
        if (id128) {
            NcclUniqueId id;
            memcpy(&id, id128, sizeof id);
            const int rc = rccl().comm_init_rank(&c->nccl, world, id, rank);
            if (rc != 0) {
                delete c;
                SKF_FAIL(SKF_E_HIP, "ncclCommInitRank failed: %s", g_rccl.error_string ? g_rccl.error_string(rc) : "?");
            }
        } else if (world != 1) {
            delete c;
            SKF_FAIL(SKF_E_INVALID, "a communicator of %d ranks needs the unique id of skf_comm_unique_id", world);
        }
        *out = c;
    });
}

int skf_comm_create_callback(int32_t rank, int32_t world, skf_collective_fn fn, void* user, skf_comm** out) {
    return guarded([&] {
        if (!out || !fn || world < 1 || rank < 0 || rank >= world) SKF_FAIL(SKF_E_INVALID, "bad rank / world / pointer");
        skf_comm* c = new skf_comm();
        c->rank = rank; c->world = world; c->fn = fn; c->user = user;
        *out = c;
    });
}

int skf_comm_create_null(int32_t rank, int32_t world, skf_comm** out) {
    return guarded([&] {
        if (!out || world < 1 || rank < 0 || rank >= world) SKF_FAIL(SKF_E_INVALID, "bad rank / world / pointer");
        skf_comm* c = new skf_comm();
        c->rank = rank; c->world = world; c->null_comm = true;
        *out = c;
    });
}

int skf_owned_rows(int32_t dtype, int64_t n_obj, int32_t part_index, int32_t part_count, int64_t* begin, int64_t* count,
                   int64_t* chunk) {
    return guarded([&] {
        if (n_obj <= 0 || part_count < 1 || part_index < 0 || part_index >= part_count || !begin || !count || !chunk)
            SKF_FAIL(SKF_E_INVALID, "bad argument");
        if (dtype != SKF_F64 && dtype != SKF_F32 && dtype != SKF_BF16) SKF_FAIL(SKF_E_INVALID, "unknown dtype %d", dtype);
        const int64_t ch = owned_chunk(dtype, n_obj, part_count);
        int64_t lo = ch * part_index, hi = lo + ch;
        if (lo > n_obj) lo = n_obj;
        if (hi > n_obj) hi = n_obj;
        *begin = lo;
        *count = hi - lo;
        *chunk = ch;
    });
}

int skf_abi_version(void) { return SKF_ABI_VERSION; }

int skf_comm_info(const skf_comm* c, int32_t* rank, int32_t* world, int32_t* transport, int32_t* transport_ranks) {
    return guarded([&] {
        if (!c) SKF_FAIL(SKF_E_INVALID, "null communicator");
        if (rank) *rank = c->rank;
        if (world) *world = c->world;
        const int kind = c->nccl ? SKF_COMM_RCCL : c->fn ? SKF_COMM_CALLBACK : c->null_comm ? SKF_COMM_NULL : SKF_COMM_SINGLE;
        if (transport) *transport = kind;
        if (transport_ranks) {
            *transport_ranks = kind == SKF_COMM_SINGLE ? 1 : kind == SKF_COMM_NULL ? 0 : c->world;
            if (c->nccl) {                     // what RCCL itself says about the communicator it built
                int n = -1, r = -1;
                if (g_rccl.comm_count && g_rccl.comm_count(c->nccl, &n) == 0) *transport_ranks = n;
                else *transport_ranks = -1;
                if (g_rccl.comm_user_rank && g_rccl.comm_user_rank(c->nccl, &r) == 0 && r != c->rank)
                    SKF_FAIL(SKF_E_STATE, "RCCL numbers this rank %d, the communicator was created as rank %d", r, c->rank);
            }
        }
    });
}

int skf_launch_count(int64_t* launches) {
    return guarded([&] {
        if (!launches) SKF_FAIL(SKF_E_INVALID, "null pointer");
        *launches = g_launches;
    });
}

int skf_split_clamps(int64_t* clamps) {
    return guarded([&] {
        if (!clamps) SKF_FAIL(SKF_E_INVALID, "null pointer");
        *clamps = g_split_clamps;
    });
}

int skf_comm_destroy(skf_comm* c) {
    return guarded([&] {
        if (!c) return;
        if (c->nccl && g_rccl.comm_destroy) (void)g_rccl.comm_destroy(c->nccl);
        delete c;
    });
}

int skf_plan_set_comm(skf_plan* p, skf_comm* comm) {
    return guarded([&] {
        if (!p) SKF_FAIL(SKF_E_INVALID, "null plan");
        if (p->variant == SKF_TRANSFORM && comm) SKF_FAIL(SKF_E_INVALID, "skf_plan_set_comm: SKF_DFMF / SKF_DFMC plans only");
        p->comm = comm;
    });
}

int skf_iterate_dist(skf_plan* p, int32_t n_iters, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (p->variant == SKF_TRANSFORM) SKF_FAIL(SKF_E_INVALID, "skf_iterate_dist: SKF_DFMF / SKF_DFMC plans only");
        if (!p->comm) SKF_FAIL(SKF_E_STATE, "no communicator attached to the plan (skf_plan_set_comm)");
        if (n_iters < 0) SKF_FAIL(SKF_E_INVALID, "n_iters < 0");
        for (size_t i = 0; i < p->types.size(); ++i)
            if (!p->types[i].set) SKF_FAIL(SKF_E_STATE, "factor of object type %zu not set", i);
        if (p->owned) {
            if (p->comm->world != p->part_count || p->comm->rank != p->part_index)
                SKF_FAIL(SKF_E_STATE, "the communicator is rank %d of %d, the plan part %d of %d", p->comm->rank, p->comm->world,
                         p->part_index, p->part_count);
            for (int it = 0; it < n_iters; ++it) iterate_owned(p, as_stream(stream));
            finalize_owned(p, as_stream(stream));
            return;
        }
        for (int it = 0; it < n_iters; ++it) iterate_dist(p, as_stream(stream));
    });
}

int skf_exchange_bytes(const skf_plan* p, int32_t world, size_t* bytes) {
    return guarded([&] {
        if (!p || !bytes || world < 1) SKF_FAIL(SKF_E_INVALID, "bad argument");
        *bytes = exchange_bytes(p, world);
    });
}

int skf_relation_sqerr(skf_plan* p, int32_t rel, double* out, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (rel < 0 || rel >= (int)p->rels.size() || !out) SKF_FAIL(SKF_E_INVALID, "bad relation index / pointer");
        hipStream_t st = as_stream(stream);
        RelState& r = p->rels[rel];
        if (r.absent) {
            SKF_HIP(hipMemsetAsync(out, 0, sizeof(double), st));
            return;
        }
        switch (form_of(r)) {
        case REL_FOLD_KNOWN: sqerr_fold_known(p, r, out, st); break;
        case REL_FOLD:       sqerr_fold(p, r, out, st); break;
        case REL_STORED:     sqerr_stored(p, r, out, st); break;
        case REL_KNOWN:      sqerr_known(p, r, out, st); break;
        case REL_DENSE:      sqerr_dense(p, r, out, st); break;
        }
    });
}

int skf_get_contraction(const skf_plan* p, int32_t rel, int32_t which, void* dst, int64_t ld, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (rel < 0 || rel >= (int)p->rels.size() || !dst || which < 0 || which > 2)
            SKF_FAIL(SKF_E_INVALID, "bad relation index / selector / pointer");
        const RelState& r = p->rels[rel];
        const TypeState& ti = p->types[r.row];
        const TypeState& tj = p->types[r.col];
        const RelForm form = form_of(r);
        if (form == REL_FOLD || form == REL_FOLD_KNOWN)
            SKF_FAIL(SKF_E_INVALID, "relation %d (SKF_REL_FOLD_CSR%s) forms neither P nor Q", rel, form == REL_FOLD_KNOWN ? " | SKF_REL_FOLD_KNOWN" : "");
        if (which == 2 && form != REL_KNOWN) SKF_FAIL(SKF_E_STATE, "relation %d forms P, not P S^T (which = 2 is for known-entries relations)", rel);
        const Slot& src = which == 0 ? r.P : which == 1 ? r.Q : r.A;
        const int64_t rows = which == 1 ? tj.n : r.nr, cols = which == 0 ? tj.c : ti.c;
        if (p->small_fused && which == 1 && r.Q.ptr) {       // the fused small-graph schedule keeps Q as shares: sum them first
            const int64_t total = rows * cols;
            if (p->f64) launch_sum_parts<double>(r.Q.ptr, r.SmQ.ptr, total, r.sm_qparts, as_stream(stream));
            else launch_sum_parts<float>(r.Q.ptr, r.SmQ.ptr, total, r.sm_qparts, as_stream(stream));
        }
        if (!src.ptr || rows <= 0) SKF_FAIL(SKF_E_STATE, "relation %d keeps no %s here", rel, which == 0 ? "P" : "Q");
        if (ld < cols) SKF_FAIL(SKF_E_INVALID, "ld too small");
        copy2d(dst, ld, src.ptr, cols, rows, cols, p->esz, as_stream(stream));
    });
}

int skf_get_relation_lists(const skf_plan* p, int32_t rel, int32_t by_col, int32_t* parts, int64_t* n_entries, int64_t* ptr,
                           int32_t* idx, void* values, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (rel < 0 || rel >= (int)p->rels.size()) SKF_FAIL(SKF_E_INVALID, "bad relation index");
        const RelState& r = p->rels[rel];
        const RelForm form = form_of(r);         // (row lists AND column lists, in parts: the two forms an iteration contracts)
        if ((form != REL_KNOWN && form != REL_STORED) || r.absent) SKF_FAIL(SKF_E_STATE, "relation %d keeps no entry lists here", rel);
        const int pc = by_col ? r.kn_pr : r.kn_pc;
        const int64_t n_out = by_col ? p->types[r.col].n : r.nr;
        if (parts) *parts = pc;
        if (n_entries) *n_entries = r.kn_nnz;
        hipStream_t st = as_stream(stream);
        const Slot& sp = by_col ? r.KcPtr : r.KrPtr;
        const Slot& si = by_col ? r.KcIdx : r.KrIdx;
        const Slot& sv = by_col ? r.KcVal : r.KrVal;
        if (ptr) SKF_HIP(hipMemcpyAsync(ptr, sp.ptr, ((size_t)n_out * pc + 1) * 8, hipMemcpyDeviceToDevice, st));
        if (idx && r.kn_nnz > 0) SKF_HIP(hipMemcpyAsync(idx, si.ptr, (size_t)r.kn_nnz * 4, hipMemcpyDeviceToDevice, st));
        if (values && r.kn_nnz > 0) SKF_HIP(hipMemcpyAsync(values, sv.ptr, (size_t)r.kn_nnz * p->esz, hipMemcpyDeviceToDevice, st));
    });
}

int skf_get_constraint_lists(const skf_plan* p, int32_t theta, int64_t* n_rows, int64_t* n_entries, int64_t* indptr, int32_t* indices,
                             void* values, void* stream) {
    return guarded([&] {
        check_bound(p);
        if (theta < 0 || theta >= (int)p->thetas.size()) SKF_FAIL(SKF_E_INVALID, "constraint %d out of range", theta);
        const ThetaState& th = p->thetas[theta];
        if (!th.sparse) SKF_FAIL(SKF_E_INVALID, "constraint %d is kept dense: no lists", theta);
        const int64_t rows = th.local ? th.ln : p->types[th.type].n;
        if (n_rows) *n_rows = rows;
        if (n_entries) *n_entries = th.nnz;
        hipStream_t st = as_stream(stream);
        if (indptr) SKF_HIP(hipMemcpyAsync(indptr, th.Rp.ptr, ((size_t)rows + 1) * 8, hipMemcpyDeviceToDevice, st));
        if (indices && th.nnz > 0) SKF_HIP(hipMemcpyAsync(indices, th.Ci.ptr, (size_t)th.nnz * 4, hipMemcpyDeviceToDevice, st));
        if (values && th.nnz > 0) SKF_HIP(hipMemcpyAsync(values, th.Vv.ptr, (size_t)th.nnz * p->esz, hipMemcpyDeviceToDevice, st));
    });
}

int skf_plan_set_profiling(skf_plan* p, int32_t enable) {
    return guarded([&] {
        if (!p) SKF_FAIL(SKF_E_INVALID, "null plan");
        p->profiling = enable != 0;
        p->ev_used = 0;
        p->prof_flops = p->prof_bytes = 0.0;
        p->prof_launches = 0;
    });
}

int skf_plan_get_profile(skf_plan* p, double* total_ms, int64_t* launches, double* flops, double* bytes) {
    return guarded([&] {
        if (!p || !total_ms || !launches || !flops || !bytes) SKF_FAIL(SKF_E_INVALID, "null argument");
        double ms = 0.0;
        for (size_t k = 0; k + 1 < p->ev_used; k += 2) {
            SKF_HIP(hipEventSynchronize(p->ev_pool[k + 1]));
            float t = 0.f;
            SKF_HIP(hipEventElapsedTime(&t, p->ev_pool[k], p->ev_pool[k + 1]));
            ms += t;
        }
        *total_ms = ms;
        *launches = p->prof_launches;
        *flops = p->prof_flops;
        *bytes = p->prof_bytes;
        p->ev_used = 0;
        p->prof_flops = p->prof_bytes = 0.0;
        p->prof_launches = 0;
    });
}

// The stand-alone products run on the CALLER's scratch, which may hold fewer slices than the time model asks for: that is
// the caller's choice, not a sizing rule of the library that fell behind -- skf_split_clamps counts the plans' launches only.
struct CallerScratch {
    int64_t keep = g_split_clamps;
    ~CallerScratch() { g_split_clamps = keep; }
};

int skf_gemm(int32_t dtype, int32_t engine, const skf_gemm_desc* d, void* workspace, size_t workspace_bytes,
             void* stream) {
    return guarded([&] {
        CallerScratch scope;
        if (!d || !d->A || !d->B || !d->C) SKF_FAIL(SKF_E_INVALID, "null argument");
        if (dtype != SKF_F64 && dtype != SKF_F32) SKF_FAIL(SKF_E_INVALID, "skf_gemm: dtype must be SKF_F64 / SKF_F32");
        if (d->epi < EPI_STORE || d->epi > EPI_MASKED_STORE) SKF_FAIL(SKF_E_INVALID, "bad epilogue");
        if ((d->epi == EPI_SPLIT_STORE || d->epi == EPI_SPLIT_ACC) && !d->C2) SKF_FAIL(SKF_E_INVALID, "C2 missing");
        if (d->epi == EPI_MASKED_STORE && !d->mask) SKF_FAIL(SKF_E_INVALID, "mask missing");
        if (d->M < 0 || d->N < 0 || d->K < 0) SKF_FAIL(SKF_E_INVALID, "negative dimension");
        GemmArgs g = gemm_args(d->A, d->sa_m, d->sa_k, d->B, d->sb_k, d->sb_n, d->C, d->ldc, d->M, d->N, d->K,
                               d->epi, d->nan_to_num);
        g.C2 = d->C2; g.ldc2 = d->ldc2 ? d->ldc2 : d->ldc;
        g.mask = d->mask; g.ldmask = d->ldmask;
        g.aop = d->aop;
        GemmTypes ty{dtype, d->a_dtype < 0 ? dtype : d->a_dtype, d->b_dtype < 0 ? dtype : d->b_dtype};
        // X^T X (one operand read both ways, plain store): a symmetric product -- the split-K form computes the tiles on / below
        // the diagonal only (GemmArgs::sym; bit for bit the full product)
        static const int sym_on = env_int("SKF_GRAM_SYM", 1) != 0;
        if (sym_on && d->A == d->B && d->M == d->N && d->sa_m == d->sb_n && d->sa_k == d->sb_k && d->epi == EPI_STORE &&
            d->aop == AOP_NONE && ty.a == ty.b)
            g.sym = 1;
        run_gemm(ty, engine, g, d->splits, workspace, workspace_bytes, as_stream(stream));
    });
}

int skf_gemm_bf16(const void* A, int64_t lda, const void* Bt, int64_t ldb, float* C, int64_t ldc, int32_t M, int32_t N,
                  int32_t Kp, int32_t splits, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] {
        CallerScratch scope;
        if (!A || !Bt || !C || M < 0 || N < 0 || Kp < 0 || ldc < N) SKF_FAIL(SKF_E_INVALID, "bad argument");
        run_gemm_bf16((const uint16_t*)A, lda, (const uint16_t*)Bt, ldb, C, ldc, M, N, Kp, splits, workspace,
                      workspace_bytes, false, as_stream(stream));
    });
}

int skf_gemm_bf16_tn(const void* A, int64_t lda, const void* Bt, int64_t ldb, float* C, int64_t ldc, int32_t M, int32_t N,
                     int32_t Kp, int32_t splits, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] {
        CallerScratch scope;
        if (!A || !Bt || !C || M < 0 || N < 0 || Kp < 0 || ldc < N) SKF_FAIL(SKF_E_INVALID, "bad argument");
        run_gemm_bf16((const uint16_t*)A, lda, (const uint16_t*)Bt, ldb, C, ldc, M, N, Kp, splits, workspace,
                      workspace_bytes, false, as_stream(stream), true);
    });
}

int skf_gemm_bits(const void* A, int64_t lda_bytes, const void* Bt, int64_t ldb, float* C, int64_t ldc, int32_t M, int32_t N,
                  int32_t Kp, int32_t transposed, int32_t splits, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] {
        CallerScratch scope;
        if (!A || !Bt || !C || M < 0 || N < 0 || Kp < 0 || ldc < N) SKF_FAIL(SKF_E_INVALID, "bad argument");
        run_gemm_bf16((const uint16_t*)A, lda_bytes, (const uint16_t*)Bt, ldb, C, ldc, M, N, Kp, splits, workspace,
                      workspace_bytes, false, as_stream(stream), transposed != 0, true);
    });
}

int skf_to_bf16(void* dst, int64_t ldd, int32_t src_dtype, const void* src, int64_t lds, int64_t rows, int64_t cols,
                int32_t transpose, void* stream) {
    return guarded([&] {
        if (!dst || !src || rows < 0 || cols < 0) SKF_FAIL(SKF_E_INVALID, "bad argument");
        if (src_dtype != SKF_F64 && src_dtype != SKF_F32 && src_dtype != SKF_BF16) SKF_FAIL(SKF_E_INVALID, "bad source dtype");
        // a row of dst holds `rows` elements when transposed, `cols` otherwise; a row of src always `cols`
        if (lds < cols || ldd < (transpose ? rows : cols))
            SKF_FAIL(SKF_E_INVALID, "skf_to_bf16: ld too small (ldd %lld, lds %lld for %lld x %lld%s)", (long long)ldd, (long long)lds,
                     (long long)rows, (long long)cols, transpose ? ", transposed" : "");
        hipStream_t st = as_stream(stream);
        if (src_dtype == SKF_F64) launch_to_bf16<double>((uint16_t*)dst, ldd, (const double*)src, lds, rows, cols, transpose != 0, st);
        else if (src_dtype == SKF_F32) launch_to_bf16<float>((uint16_t*)dst, ldd, (const float*)src, lds, rows, cols, transpose != 0, st);
        else if (src_dtype == SKF_BF16) launch_to_bf16<uint16_t>((uint16_t*)dst, ldd, (const uint16_t*)src, lds, rows, cols, transpose != 0, st);
        else SKF_FAIL(SKF_E_INVALID, "bad source dtype");
    });
}

int skf_fold_lists(int32_t dtype, const int64_t* indptr, const int32_t* indices, const void* values, int64_t n_out, const void* T,
                   int64_t ldt, int32_t c, void* Ec, int64_t lde, void* Dc, int64_t ldd, void* stream) {
    return guarded([&] {
        if (dtype != SKF_F64 && dtype != SKF_F32) SKF_FAIL(SKF_E_INVALID, "skf_fold_lists: dtype must be SKF_F64 / SKF_F32");
        if (!indptr || !indices || !values || !T || !Ec || !Dc) SKF_FAIL(SKF_E_INVALID, "null argument");
        if (n_out < 0 || n_out > 2000000000LL || c < 1 || c > 1024) SKF_FAIL(SKF_E_INVALID, "skf_fold_lists: n_out %lld / width %d", (long long)n_out, c);
        if (ldt < c || lde < c || ldd < c) SKF_FAIL(SKF_E_INVALID, "ld too small");
        if (dtype == SKF_F64)
            launch_fold_lists<double>(indptr, (const int*)indices, values, n_out, T, ldt, c, Ec, lde, Dc, ldd, as_stream(stream));
        else
            launch_fold_lists<float>(indptr, (const int*)indices, values, n_out, T, ldt, c, Ec, lde, Dc, ldd, as_stream(stream));
    });
}

int skf_fold_known_pass(int32_t dtype, const int64_t* indptr, const int32_t* indices, const void* values, int64_t n_out, const void* G,
                        int64_t ldg, const void* T, int64_t ldt, int32_t c, const void* X, int64_t ldx, void* E, int64_t lde, void* D,
                        int64_t ldd, void* stream) {
    return guarded([&] {
        if (dtype != SKF_F64 && dtype != SKF_F32) SKF_FAIL(SKF_E_INVALID, "skf_fold_known_pass: dtype must be SKF_F64 / SKF_F32");
        if (!indptr || !indices || !values || !G || !T || !E || !D) SKF_FAIL(SKF_E_INVALID, "null argument");
        if (n_out < 0 || n_out > 2000000000LL || c < 1 || c > 1024)
            SKF_FAIL(SKF_E_INVALID, "skf_fold_known_pass: n_out %lld / width %d", (long long)n_out, c);
        if (ldg < c || ldt < c || lde < c || ldd < c || (X && ldx < c)) SKF_FAIL(SKF_E_INVALID, "ld too small");
        if (dtype == SKF_F64)
            launch_fold_known<double>(indptr, (const int*)indices, values, n_out, G, ldg, T, ldt, c, X, ldx, E, lde, D, ldd, nullptr,
                                      as_stream(stream));
        else
            launch_fold_known<float>(indptr, (const int*)indices, values, n_out, G, ldg, T, ldt, c, X, ldx, E, lde, D, ldd, nullptr,
                                     as_stream(stream));
    });
}

int skf_pinv_sym_workspace_bytes(int32_t n, size_t* bytes) {
    return guarded([&] {
        if (n <= 0 || n > EIGH_MAXN - 1 || !bytes) SKF_FAIL(SKF_E_INVALID, "bad order");
        *bytes = pinv_sym_layout(n).total;
    });
}

int skf_pinv_sym(int32_t dtype, const void* A, int64_t lda, void* K, int64_t ldk, int32_t n, void* ws,
                 size_t ws_bytes, void* stream) {
    return guarded([&] {
        size_t need = 0;
        if (skf_pinv_sym_workspace_bytes(n, &need) != SKF_OK) SKF_FAIL(SKF_E_INVALID, "bad order %d", n);
        if (!A || !K || !ws || ws_bytes < need) SKF_FAIL(SKF_E_WORKSPACE, "pinv workspace too small / null pointer");
        if (dtype != SKF_F64 && dtype != SKF_F32) SKF_FAIL(SKF_E_INVALID, "bad dtype");
        const int np = (n + 1) / 2 * 2;
        const PinvSymLayout l = pinv_sym_layout(n);
        char* base = (char*)ws;
        const Switches sw = Switches::read();          // stand-alone operator: no plan to hold them
        PinvBatch pb;
        memset(&pb, 0, sizeof pb);
        pb.gram[0] = A; pb.ldg[0] = lda;
        pb.K[0] = K; pb.ldk[0] = ldk;
        pb.c[0] = n; pb.n_pad[0] = np;
        PinvRun r;
        r.sw = &sw; r.engine = SKF_ENGINE_MFMA;
        r.e.A = (double*)(base + l.A); r.e.V = (double*)(base + l.V); r.e.Vs = (double*)(base + l.Vs);
        r.e.w = (double*)(base + l.w); r.e.stride = (int64_t)np * np; r.e.wstride = np;
        r.e.n = (const int*)(base + l.n); r.e.n_orig = (const int*)(base + l.n_orig); r.e.chol_ok = (int*)(base + l.ok);
        r.e.max_sweeps = 30;
        r.pb = &pb; r.nb = 1; r.max_c = n; r.max_pad = np;
        r.lds_order = np;
        r.dtype = dtype;
        r.k_direct = dtype == SKF_F64 && ldk == n;     // else: Cholesky inverse + unpack into the caller's type and stride
        r.defl_scratch = n > SWEEP_MAXN ? base + l.defl : nullptr;
        r.write_orders = true;
        run_pinv(r, as_stream(stream));
    });
}

int skf_fill_uniform(int32_t dtype, void* dst, int64_t rows, int64_t cols, int64_t ld, uint64_t seed, double scale,
                     double shift, void* stream) {
    return guarded([&] {
        if (!dst || rows < 0 || cols < 0 || ld < cols) SKF_FAIL(SKF_E_INVALID, "bad argument");
        hipStream_t st = as_stream(stream);
        const int grid = elem_grid(rows * cols);
        if (dtype == SKF_F64)
            hipLaunchKernelGGL((fill_uniform_kernel<double>), dim3(grid), dim3(256), 0, st, (double*)dst, rows, cols, ld,
                               seed, scale, shift);
        else if (dtype == SKF_F32)
            hipLaunchKernelGGL((fill_uniform_kernel<float>), dim3(grid), dim3(256), 0, st, (float*)dst, rows, cols, ld,
                               seed, scale, shift);
        else if (dtype == SKF_BF16)
            hipLaunchKernelGGL((fill_uniform_kernel<uint16_t>), dim3(grid), dim3(256), 0, st, (uint16_t*)dst, rows, cols,
                               ld, seed, scale, shift);
        else
            SKF_FAIL(SKF_E_INVALID, "bad dtype");
        check_launch("fill_uniform");
    });
}

int skf_fill_unknown_workspace_bytes(int64_t rows, int64_t cols, size_t* bytes) {
    return guarded([&] {
        if (rows < 0 || cols < 0 || !bytes) SKF_FAIL(SKF_E_INVALID, "bad argument");
        *bytes = (size_t)(2 * rows + 2 * cols + 2) * sizeof(double);
    });
}

int skf_fill_unknown(int32_t dtype, void* data, int64_t ld, int64_t rows, int64_t cols, const uint8_t* mask, int64_t mask_ld,
                     int32_t strategy, double value, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] {
        if (!data || rows < 0 || cols < 0 || ld < cols || (mask && mask_ld < cols)) SKF_FAIL(SKF_E_INVALID, "bad argument");
        if (dtype != SKF_F64 && dtype != SKF_F32) SKF_FAIL(SKF_E_INVALID, "skf_fill_unknown: dtype must be SKF_F64 / SKF_F32");
        if (strategy < FILL_MEAN || strategy > FILL_CONST) SKF_FAIL(SKF_E_INVALID, "unknown fill strategy %d", strategy);
        size_t need = 0;
        skf_fill_unknown_workspace_bytes(rows, cols, &need);
        if (!workspace || workspace_bytes < need) SKF_FAIL(SKF_E_WORKSPACE, "fill workspace too small / null");
        if (rows == 0 || cols == 0) return;
        hipStream_t st = as_stream(stream);
        double* stats = (double*)workspace;
        const int rgrid = wave_grid(rows);
        if (dtype == SKF_F64) {
            double* X = (double*)data;
            if (strategy != FILL_CONST) {
                hipLaunchKernelGGL((fill_row_stats_kernel<double>), dim3(rgrid), dim3(256), 0, st, X, ld, rows, cols, mask, mask_ld, stats);
                if (strategy == FILL_COL_MEAN)
                    hipLaunchKernelGGL((fill_col_stats_kernel<double>), dim3(elem_grid(cols)), dim3(256), 0, st, X, ld, rows, cols, mask, mask_ld, stats);
                hipLaunchKernelGGL(fill_total_kernel, dim3(1), dim3(256), 0, st, rows, cols, stats);
            }
            hipLaunchKernelGGL((fill_apply_kernel<double>), dim3(elem_grid(rows * cols)), dim3(256), 0, st, X, ld, rows, cols, mask,
                               mask_ld, stats, strategy, value);
        } else {
            float* X = (float*)data;
            if (strategy != FILL_CONST) {
                hipLaunchKernelGGL((fill_row_stats_kernel<float>), dim3(rgrid), dim3(256), 0, st, X, ld, rows, cols, mask, mask_ld, stats);
                if (strategy == FILL_COL_MEAN)
                    hipLaunchKernelGGL((fill_col_stats_kernel<float>), dim3(elem_grid(cols)), dim3(256), 0, st, X, ld, rows, cols, mask, mask_ld, stats);
                hipLaunchKernelGGL(fill_total_kernel, dim3(1), dim3(256), 0, st, rows, cols, stats);
            }
            hipLaunchKernelGGL((fill_apply_kernel<float>), dim3(elem_grid(rows * cols)), dim3(256), 0, st, X, ld, rows, cols, mask,
                               mask_ld, stats, strategy, value);
        }
        check_launch("fill_unknown");
    });
}

int skf_cast(int32_t dst_dtype, void* dst, int64_t ldd, int32_t src_dtype, const void* src, int64_t lds, int64_t rows,
             int64_t cols, void* stream) {
    return guarded([&] {
        if (!dst || !src || rows < 0 || cols < 0) SKF_FAIL(SKF_E_INVALID, "bad argument");
        if (ldd < cols || lds < cols) SKF_FAIL(SKF_E_INVALID, "skf_cast: ld too small (ldd %lld, lds %lld for %lld columns)",
                                               (long long)ldd, (long long)lds, (long long)cols);
        hipStream_t st = as_stream(stream);
        const int grid = elem_grid(rows * cols);
        if (dst_dtype == SKF_F32 && src_dtype == SKF_F64)
            hipLaunchKernelGGL((cast_kernel<float, double>), dim3(grid), dim3(256), 0, st, (float*)dst, ldd,
                               (const double*)src, lds, rows, cols);
        else if (dst_dtype == SKF_F64 && src_dtype == SKF_F32)
            hipLaunchKernelGGL((cast_kernel<double, float>), dim3(grid), dim3(256), 0, st, (double*)dst, ldd,
                               (const float*)src, lds, rows, cols);
        else if (dst_dtype == SKF_F32 && src_dtype == SKF_F32)
            hipLaunchKernelGGL((cast_kernel<float, float>), dim3(grid), dim3(256), 0, st, (float*)dst, ldd,
                               (const float*)src, lds, rows, cols);
        else if (dst_dtype == SKF_F64 && src_dtype == SKF_F64)
            hipLaunchKernelGGL((cast_kernel<double, double>), dim3(grid), dim3(256), 0, st, (double*)dst, ldd,
                               (const double*)src, lds, rows, cols);
        else
            SKF_FAIL(SKF_E_INVALID, "unsupported cast %d -> %d", src_dtype, dst_dtype);
        check_launch("cast");
    });
}

}  // extern "C"
