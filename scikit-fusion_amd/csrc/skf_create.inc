// skf_create.inc -- part of the one translation unit skf_api.hip (textually included there, behind `using namespace skf`;
// not a header of its own): plan creation, in the order skf_plan_create calls its five steps --
//   plan_describe_types -> plan_describe_relations -> plan_decide_lists -> plan_describe_constraints -> plan_layout.
// The first four check the descriptors and say what the plan holds (every refusal of skf_plan_create past its argument
// check is here, and the order of the lines is the order in which they answer: tests/plan_create_cases.py); the fifth
// hands out the workspace.  Nothing here makes a HIP call.
//
// The layout lists the products of a plan by hand: each form of a relation (RelForm, skf_plan.inc) has ONE function that
// adds its slots and names the split-K products and error partials of its launches, to be read against the functions of
// skf_stages.inc / skf_steps.inc its header names.  add_slot hands out offsets in call order and the distributed
// iterations reduce several ranges as one buffer, so the ORDER of the add_slot calls is behaviour.

// ---- 1. the options and the object types: sizes, ranks, and the rows of every type this process holds ----------------------
static void plan_describe_types(skf_plan* p, int32_t n_types, const skf_type_desc* types, const skf_options* opt) {
    p->dtype = opt->dtype;
    p->variant = opt->variant;
    p->engine = opt->engine;
    p->f64 = (opt->dtype == SKF_F64);
    p->bf16 = (opt->dtype == SKF_BF16);
    p->esz = p->f64 ? 8 : 4;
    p->mt = p->f64 ? SKF_F64 : SKF_F32;
    p->target = opt->target_type;
    if (p->variant == SKF_TRANSFORM && (p->target < 0 || p->target >= n_types))
        SKF_FAIL(SKF_E_INVALID, "target type %d out of range", p->target);
    p->types.resize(n_types);
    for (int i = 0; i < n_types; ++i) {
        if (types[i].n_obj <= 0 || types[i].rank <= 0 || types[i].rank > EIGH_MAXN - 1)
            SKF_FAIL(SKF_E_INVALID, "object type %d: n_obj=%lld rank=%d invalid", i, (long long)types[i].n_obj,
                     types[i].rank);
        if (types[i].n_obj > 2000000000LL) SKF_FAIL(SKF_E_INVALID, "object type %d too large", i);
        TypeState& t = p->types[i];
        t.n = t.tn = t.n_alloc = types[i].n_obj;
        t.c = types[i].rank;
        t.n_pad = (t.c + 1) / 2 * 2;
        const bool own = (opt->flags & SKF_OPT_OWNED_ROWS) != 0;      // the rows this process owns (skf_owned_rows)
        if (own && (opt->part_count < 1 || opt->part_index < 0 || opt->part_index >= opt->part_count))
            SKF_FAIL(SKF_E_INVALID, "SKF_OPT_OWNED_ROWS: part_index %d outside [0, %d)", opt->part_index, opt->part_count);
        if (!own && opt->part_count <= 1) continue;
        if (opt->part_index < 0 || opt->part_index >= opt->part_count)
            SKF_FAIL(SKF_E_INVALID, "part_index %d outside [0, %d)", opt->part_index, opt->part_count);
        // (without ownership: even shares of the rows, boundaries at multiples of 64)
        const int64_t step = own ? owned_chunk(opt->dtype, t.n, opt->part_count)
                                 : ((t.n + opt->part_count - 1) / opt->part_count + 63) / 64 * 64;
        t.t0 = std::min(step * opt->part_index, t.n);
        t.tn = std::min(step * opt->part_index + step, t.n) - t.t0;
        if (own) {
            t.chunk = step;
            t.n_alloc = step * opt->part_count;
        }
    }
    if (opt->part_count > 1) p->sliced = true;
    if ((opt->flags & SKF_OPT_THETA_OWNED_ROWS) && !(opt->flags & SKF_OPT_OWNED_ROWS))
        SKF_FAIL(SKF_E_INVALID, "SKF_OPT_THETA_OWNED_ROWS needs SKF_OPT_OWNED_ROWS");
    p->theta_owned = (opt->flags & SKF_OPT_THETA_OWNED_ROWS) != 0;
    if (opt->flags & SKF_OPT_OWNED_ROWS) {
        if (p->variant == SKF_TRANSFORM) SKF_FAIL(SKF_E_INVALID, "SKF_OPT_OWNED_ROWS is for SKF_DFMF / SKF_DFMC plans");
        p->owned = p->sliced = true;
        p->part_index = opt->part_index;
        p->part_count = opt->part_count;
    }
}

// ---- 2. the relations: which form each one comes in, and whether that form goes with the plan -----------------------------

// what the entry lists take: gathered vectors of at most 64 * SRP_MAXREP numbers (skf_known.h), positions in 32 bits
constexpr int LIST_MAX_RANK = 64 * SRP_MAXREP;
constexpr int64_t LIST_MAX_ENTRIES = 2000000000LL;

// the flags of relation `r` (read off into `s` already): which go together, with which plan, and with or without a matrix
static void check_relation(skf_plan* p, int r, const skf_relation_desc& d, const RelState& s) {
    const bool matrix = d.data || d.mask || (d.flags & (SKF_REL_MASKED | SKF_REL_MASK_BITS));    // anything of a dense form: a list form takes none
    if (s.kn_csr && p->variant != SKF_DFMC) SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_KNOWN_CSR needs SKF_DFMC", r);
    if (s.kn_csr && (d.data || d.mask)) SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_KNOWN_CSR takes no data / mask", r);
    if (s.sp0 && s.kn_csr) SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_KNOWN_CSR and SKF_REL_SPARSE_CSR exclude each other", r);
    if (s.sp0 && p->variant == SKF_TRANSFORM) SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_SPARSE_CSR is for SKF_DFMF / SKF_DFMC plans", r);
    if (s.sp0 && matrix) SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_SPARSE_CSR takes no data / mask", r);
    if (s.fold && p->variant != SKF_TRANSFORM) SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_FOLD_CSR is for SKF_TRANSFORM plans", r);
    if (s.fold && (s.kn_csr || s.sp0))
        SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_FOLD_CSR excludes SKF_REL_KNOWN_CSR / SKF_REL_SPARSE_CSR", r);
    if (s.fold_known && p->variant != SKF_TRANSFORM)
        SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_FOLD_KNOWN is for SKF_TRANSFORM plans", r);
    if (s.fold_known && !s.fold) SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_FOLD_KNOWN goes with SKF_REL_FOLD_CSR", r);
    if (s.fill && (!s.sp0 || s.absent || p->owned || p->variant == SKF_TRANSFORM))
        SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_FILL_RANK1 goes with SKF_REL_SPARSE_CSR on SKF_DFMF / SKF_DFMC plans of whole "
                 "relations (no SKF_OPT_OWNED_ROWS, no fold-in)", r);
    if (s.fold && matrix) SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_FOLD_CSR takes no data / mask", r);
    if (!s.absent && !s.kn_csr && !s.sp0 && !s.fold && (!d.data || d.ld < p->types[d.col_type].n))
        SKF_FAIL(SKF_E_INVALID, "relation %d: dimension mismatch (ld %lld < %lld columns)", r, (long long)d.ld,
                 (long long)p->types[d.col_type].n);
    // ... then the rows this plan holds, its mask, the plan's target.  A row block makes the plan a sliced one.
    const int64_t n_row_type = p->types[d.row_type].n, n_col_type = p->types[d.col_type].n;
    if (d.row_begin < 0 || d.n_rows < 0 || d.row_begin + d.n_rows > n_row_type)
        SKF_FAIL(SKF_E_INVALID, "relation %d: row block [%lld, +%lld) outside the %lld objects of its row type",
                 r, (long long)d.row_begin, (long long)d.n_rows, (long long)n_row_type);
    const bool block = s.absent || (d.n_rows > 0 && d.n_rows < n_row_type) || (d.flags & SKF_REL_NO_COL_SIDE);
    // (SKF_OPT_OWNED_ROWS: the CSR of the owned rows, over all columns -- held to the owned range by the caller, like a dense block)
    if (block && (s.kn_csr || s.sp0) && !p->owned)
        SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_KNOWN_CSR / SKF_REL_SPARSE_CSR relations are whole relations "
                 "(or the owned rows of a SKF_OPT_OWNED_ROWS plan)", r);
    if (block && s.fold) SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_FOLD_CSR relations are whole relations", r);
    if (block && p->variant == SKF_TRANSFORM)
        SKF_FAIL(SKF_E_INVALID, "relation %d: row blocks are for SKF_DFMF / SKF_DFMC plans", r);
    if (block && p->bf16 && d.row_begin % 64 != 0)
        SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_BF16 row blocks must start at a multiple of 64", r);
    if (block) p->sliced = true;
    if ((d.mask || (d.flags & SKF_REL_MASKED)) && p->variant != SKF_DFMC)
        SKF_FAIL(SKF_E_INVALID, "relation %d: masks need SKF_DFMC", r);
    if (d.mask && d.mask_ld < ((d.flags & SKF_REL_MASK_BITS) ? (n_col_type + 7) / 8 : n_col_type))
        SKF_FAIL(SKF_E_INVALID, "relation %d: mask ld", r);
    if (p->variant == SKF_TRANSFORM && d.row_type != p->target && d.col_type != p->target)
        SKF_FAIL(SKF_E_INVALID, "relation %d must include the target object type", r);
}

// ONE relation: its flags read off once, the refusals (check_relation), then what the plan keeps of the descriptor
// (a refused plan is thrown away whole, so what `s` holds by then is of no account)
static void plan_describe_relation(skf_plan* p, int32_t n_types, int r, const skf_relation_desc& d) {
    if (d.row_type < 0 || d.row_type >= n_types || d.col_type < 0 || d.col_type >= n_types)
        SKF_FAIL(SKF_E_INVALID, "relation %d: type index out of range", r);
    if (d.row_type == d.col_type) SKF_FAIL(SKF_E_INVALID, "relation %d: row type == column type (pass it as a constraint)", r);
    RelState& s = p->rels[r];
    s.absent = (d.flags & SKF_REL_ABSENT) != 0;
    s.kn_csr = (d.flags & SKF_REL_KNOWN_CSR) != 0;            // the known entries as CSR: no dense form, no mask
    s.sp0 = (d.flags & SKF_REL_SPARSE_CSR) != 0;              // the stored entries as CSR, every other entry zero
    s.fold = (d.flags & SKF_REL_FOLD_CSR) != 0;               // fold-in: one set of lists along the target, no P / Q
    s.fold_known = (d.flags & SKF_REL_FOLD_KNOWN) != 0;       // ... stored = known, every other entry unknown
    s.fill = (d.flags & SKF_REL_FILL_RANK1) != 0;             // F = a b^T + D: a filled relation with missing values
    check_relation(p, r, d, s);
    const bool lists = s.kn_csr || s.sp0 || s.fold;           // handed over by skf_plan_set_known_entries: no dense form in any type
    s.row = d.row_type; s.col = d.col_type;
    s.R_in = d.data; s.ld_in = d.ld; s.mask = d.mask; s.ldmask = d.mask_ld;
    s.mask_is_bits = (d.flags & SKF_REL_MASK_BITS) != 0;
    s.binary = p->bf16 && (d.flags & SKF_REL_BINARY) != 0 && !d.mask && !s.absent && !s.sp0 && !s.fold;
    s.R = d.data; s.ldr = d.ld;
    s.r0 = s.absent ? 0 : d.row_begin;
    s.nr = s.absent ? 0 : (d.n_rows > 0 ? d.n_rows : p->types[d.row_type].n - d.row_begin);
    s.col_side = (d.flags & SKF_REL_NO_COL_SIDE) == 0;
    s.masked = d.mask != nullptr || (d.flags & SKF_REL_MASKED) != 0 || s.kn_csr;
    if (s.absent) s.mask = nullptr;
    if (s.absent || lists) s.R_in = s.R = nullptr;
    if (p->owned) {         // the block of a relation is the owned range of its row type, nothing else
        const TypeState& ti = p->types[d.row_type];
        if (ti.tn == 0 ? !s.absent : (s.absent || s.r0 != ti.t0 || s.nr != ti.tn))
            SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_OPT_OWNED_ROWS wants the rows [%lld, +%lld) of its row type here (skf_owned_rows)",
                     r, (long long)ti.t0, (long long)ti.tn);
        s.col_side = true;  // every process adds the column-side terms of ITS rows of the column type
    }
    if (d.known_bound < 0) SKF_FAIL(SKF_E_INVALID, "relation %d: negative bound on the known entries", r);
    s.kn_cap = (lists || (s.mask && p->variant == SKF_DFMC)) ? d.known_bound : 0;      // (lists: the bound is the count)
    if (s.fold && (p->types[d.row_type].c > 1024 || p->types[d.col_type].c > 1024 || d.known_bound > LIST_MAX_ENTRIES))
        SKF_FAIL(SKF_E_INVALID, "relation %d: SKF_REL_FOLD_CSR beyond the list limits (a rank above 1024 or %lld > 2e9 entries)",
                 r, (long long)d.known_bound);
}

static void plan_describe_relations(skf_plan* p, int32_t n_types, int32_t n_relations, const skf_relation_desc* relations) {
    p->rels.resize(n_relations);
    for (int r = 0; r < n_relations; ++r) plan_describe_relation(p, n_types, r, relations[r]);
}

// ---- 3. which relations are kept as lists, and in how many parts -----------------------------------------------------------
// Masked relations with few known entries are kept as lists of those entries (skf_known.h).  The three passes over the
// lists gather rank_row-wide vectors -- ~70 ps per entry at rank 128 against ~2.2 ps per CELL for the four passes of
// the dense path over the completed relation (config 5, bf16) -- hence: known share * rank_row <= 4 (1/32 at rank
// 128).  SKF_DFMC_SPARSE=0: never; =1: whenever a bound is given (up to a quarter of the relation).  Plans with row
// blocks keep the dense form.
//
// Parts of the lists (skf_known.h): with srp_bf16_v6_kernel the passes are no longer bound by instruction issue and
// pinning slices of the gathered matrix to XCDs pays (profiles/r03_srp_v6.txt: 25.6 MB of user factors, 8 parts:
// 1.75 -> 1.10 ms; 10 MB, 4 parts: 1.41 -> 1.25 ms) -- the smallest power of two that brings a slice under the
// 4 MiB L2 of an XCD, as long as a segment still holds a batch of entries.  Other engines / widths: 1 (their
// kernels are issue-bound; measured neutral in round 3).  SKF_KNOWN_PARTS=1|2|4|8 overrides.

// parts by the size of the gathered matrix alone: n_in vectors of c bf16 numbers
static int by_bytes(const Switches& sw, int64_t n_in, int c) {
    if (sw.known_parts) return sw.known_parts;
    int q = 1;
    while (q < 8 && (double)n_in * c * 2.0 / q > 3.5 * 1048576.0) q *= 2;
    return q;
}
// ... of lists of `cap` entries over n_out lines: as long as a segment still holds a batch of entries
static int pick_parts(const skf_plan* p, const Switches& sw, int64_t n_in, int64_t n_out, int ci, int64_t cap) {
    if (sw.known_parts) return sw.known_parts;
    if (!p->bf16 || (ci != 128 && ci != 256)) return 1;
    int q = by_bytes(sw, n_in, ci);
    while (q > 1 && (double)cap / ((double)n_out * q) < 64.0) q /= 2;
    return q;
}
// the parts of a relation's lists: the row lists gather vectors of c_rl numbers of the column objects, the column lists
// vectors of c_cl numbers of the row objects; a part covers whole blocks of 64 objects of the gathered side
static void set_parts(const skf_plan* p, const Switches& sw, RelState& s, int c_rl, int c_cl) {
    const int64_t cols = p->types[s.col].n;
    s.kn_pc = pick_parts(p, sw, cols, s.nr, c_rl, s.kn_cap);
    s.kn_pr = pick_parts(p, sw, s.nr, cols, c_cl, s.kn_cap);
    s.kn_pw = ((cols + s.kn_pc - 1) / s.kn_pc + 63) / 64 * 64;
    s.kn_ph = ((s.nr + s.kn_pr - 1) / s.kn_pr + 63) / 64 * 64;
}

// One decision per form.  (form_of before `kn` is set: REL_FOLD*, REL_STORED are final, REL_DENSE is "a matrix or known entries".)
static void plan_decide_lists(skf_plan* p, const skf_relation_desc* relations) {
    const Switches sw = Switches::read();          // (plan creation: the plan's own copy is read when its workspace is bound)
    for (size_t rk = 0; rk < p->rels.size(); ++rk) {
        RelState& s = p->rels[rk];
        TypeState &ti = p->types[s.row], &tj = p->types[s.col];
        const RelForm form = form_of(s);
        const char* const flag = s.sp0 ? "SKF_REL_SPARSE_CSR" : "SKF_REL_KNOWN_CSR";
        const bool beyond = ti.c > LIST_MAX_RANK || s.kn_cap > LIST_MAX_ENTRIES;     // what the lists of the row type's vectors take
        if (form == REL_FOLD || form == REL_FOLD_KNOWN) continue;      // one set of lists as handed over: no parts, nothing decided
        if ((s.sp0 || s.kn_csr) && p->sliced && !p->owned)
            SKF_FAIL(SKF_E_INVALID, "relation %zu: %s is for plans of whole relations or of owned rows", rk, flag);
        if (form == REL_STORED) {
            // valued lists whatever the density (the caller chose the form; no dense one to fall back on).  P gathers
            // rank_col-wide rows of G_j through the row lists, Q rank_row-wide rows of G_i through the column lists
            if (beyond || tj.c > LIST_MAX_RANK)
                SKF_FAIL(SKF_E_INVALID, "relation %zu: SKF_REL_SPARSE_CSR beyond the list limits (a rank above %d or %lld > 2e9 entries)",
                         rk, LIST_MAX_RANK, (long long)s.kn_cap);
            set_parts(p, sw, s, tj.c, ti.c);
            if (p->bf16) ti.need_rows = tj.need_rows = true;
            continue;
        }
        bool lists;
        if (s.kn_csr) {
            // known entries as CSR: lists whatever the share (no dense form to fall back on); the parts follow from the exact
            // count (SKF_OPT_OWNED_ROWS: the slice of the owned rows; from here on a masked row block flagged SKF_REL_KNOWN_LISTS)
            if (beyond)
                SKF_FAIL(SKF_E_INVALID, "relation %zu: SKF_REL_KNOWN_CSR beyond the list limits (rank %d > %d or %lld > 2e9 entries)",
                         rk, ti.c, LIST_MAX_RANK, (long long)s.kn_cap);
            lists = true;
        } else if (p->owned) {
            // ownership-aligned row blocks: the caller decided for ALL processes alike (SKF_REL_KNOWN_LISTS); a process
            // without rows of the relation keeps the flag -- it adds the dense part of Q on ITS rows of the column type
            lists = (relations[rk].flags & SKF_REL_KNOWN_LISTS) != 0 && s.masked && p->variant == SKF_DFMC;
            if (lists && (beyond || (!s.absent && s.kn_cap <= 0)))
                SKF_FAIL(SKF_E_INVALID, "relation %zu: SKF_REL_KNOWN_LISTS needs a bound on the known entries of the local rows", rk);
        } else {
            // a mask with a bound: by the share of the known entries (never on a plan of row blocks)
            const double cells = (double)s.nr * (double)tj.n, share = cells > 0 ? (double)s.kn_cap / cells : 1.0;
            const int mode = sw.dfmc_sparse;
            lists = s.kn_cap > 0 && !(p->sliced || mode == 0 || share > 0.25 || (mode != 1 && share * ti.c > 4.0) || beyond);
        }
        if (!lists) { s.kn_cap = 0; continue; }
        s.kn = true;                        // REL_KNOWN from here on
        if (s.absent) continue;             // (no lists here: only the flag)
        set_parts(p, sw, s, ti.c, ti.c);    // (both sides gather rank_row-wide vectors: T = G_j S^T and G_i)
        ti.keep_prev = tj.keep_prev = true;
        if (p->bf16) ti.need_rows = true;   // the column lists gather the row type's bf16 rows
    }
    // sparse 0/1 relations as lists over bf16 factor rows (srp_bf16_v6_kernel<.., SRP_ONES>): both ranks 64 / 128 / 256
    auto gather_rank = [](int c) { return c == 64 || c == 128 || c == 256; };
    for (RelState& s : p->rels) {
        TypeState &ti = p->types[s.row], &tj = p->types[s.col];
        s.sp_gather = p->bf16 && s.binary && !s.masked && !s.absent && gather_rank(ti.c) && gather_rank(tj.c);
        if (!s.sp_gather) continue;
        ti.need_rows = tj.need_rows = true;
        // parts by the size of the gathered matrix alone (the number of ones is known at bind time, which may lower them)
        s.sp_pc = by_bytes(sw, tj.n, tj.c);    // P: rows of G_j by the column index
        s.sp_pr = by_bytes(sw, ti.n, ti.c);    // Q: rows of G_i by the row index
    }
}

// ---- 4. the constraints, and what the owners of rows keep of the other owners' factors --------------------------------------

static void plan_describe_constraints(skf_plan* p, int32_t n_types, int32_t n_thetas, const skf_theta_desc* thetas) {
    p->thetas.resize(n_thetas);
    for (int t = 0; t < n_thetas; ++t) {
        const skf_theta_desc& d = thetas[t];
        ThetaState& th = p->thetas[t];
        if (d.type < 0 || d.type >= n_types || (d.data && d.ld < p->types[d.type].n))
            SKF_FAIL(SKF_E_INVALID, "constraint %d invalid", t);
        if (p->variant == SKF_TRANSFORM && d.type != p->target)
            SKF_FAIL(SKF_E_INVALID, "constraint %d must be on the target object type", t);
        th.type = d.type;
        th.data = d.data;
        th.ld = d.ld;
        const int64_t nn = p->types[d.type].n;
        if (d.nnz < 0) SKF_FAIL(SKF_E_INVALID, "constraint %d: negative non-zero bound", t);
        if (!d.data) {      // the CSR of its stored entries (skf_plan_set_constraint_entries): no dense form in any type
            // (SKF_OPT_THETA_OWNED_ROWS on an owned plan: the CSR of the owned rows of the type, over all columns)
            const bool local = p->owned && p->theta_owned;
            if (p->sliced && !local)
                SKF_FAIL(SKF_E_INVALID, "constraint %d: a constraint given as its entries is for plans of whole relations "
                         "(no row blocks, slices or SKF_OPT_OWNED_ROWS)", t);
            if (d.nnz > LIST_MAX_ENTRIES) SKF_FAIL(SKF_E_INVALID, "constraint %d: %lld > 2e9 entries", t, (long long)d.nnz);
            th.entries = th.sparse = true;
            th.nnz_cap = d.nnz;
            th.local = local;
            th.l0 = p->types[d.type].t0;
            th.ln = p->types[d.type].tn;
        } else if (d.nnz > 0 && d.nnz <= nn * nn / SKF_THETA_SPARSE_DIV) {
            th.sparse = true;
            th.nnz_cap = d.nnz;
        }
    }
    // hub rows of the sparse constraints: the threshold, and a bound on the segments they can be cut into -- a row of L > H
    // entries gives ceil(L / H) < 2 L / H segments, all hub rows together fewer than 2 nnz / H
    const int hub_row = Switches::read().theta_hub_row;          // (plan creation: the layout's scratch is sized from it)
    for (ThetaState& th : p->thetas) {
        if (!th.sparse || hub_row <= 0 || th.nnz_cap <= hub_row) continue;
        th.hub_row = hub_row;
        th.seg_cap = 2 * th.nnz_cap / hub_row + 1;
    }
    if (!p->owned) return;
    // SKF_BF16: the other owners' rows of a factor are read as bf16 operands only -- unless a constraint on the type
    // multiplies the f32 rows (theta_spmm_kernel / dense Theta).  Every type keeps its bf16 rows (the gathered form).
    for (TypeState& t : p->types) {
        t.gather_master = !p->bf16;
        if (p->bf16) t.need_rows = true;
    }
    for (const ThetaState& th : p->thetas) p->types[th.type].gather_master = true;
    // ... and the types of a masked relation (the same on every process, whatever it holds of the relation): the
    // known-entry form multiplies the f32 rows of both factors (cross-Gram matrices, T = G_j S^T, the dense part of Q)
    for (const RelState& r : p->rels)
        if (r.masked) p->types[r.row].gather_master = p->types[r.col].gather_master = true;
}

// ---- 5. workspace layout: n-sized buffers in the master type, every c x c matrix in f64 -------------------------------------

// The running maxima of the layout: the scratch every launch shares is sized from them at the end (layout_shared_scratch).
// Split-K scratch: every product that runs on it is sized by the decision its launch takes (kind_part_bytes -> slice_gemm).
struct LayoutMax {
    const skf_plan* p;
    // split-K partials of the main / of the second stream; ... of the Gram products of all types side by side (gram_all);
    // partial outputs of the parted passes over the ones of 0/1 relations; error partials (slot 0 collects the trace term, a
    // pass writes behind it); SKF_BF16: the n x c product of a dense constraint; the largest eigen order
    size_t part_bytes = 0, aux_bytes = 0, gram_group = 0, sp_part_bytes = 0, sq_elems = 1, theta_tmp_bytes = 0;
    int maxn = 2;
    size_t want_part(const ProductKind& k, int64_t M, int64_t N, int64_t K, bool aux_too = false) {
        const size_t need = kind_part_bytes(p, k, M, N, K);
        part_bytes = std::max(part_bytes, need);
        if (aux_too) aux_bytes = std::max(aux_bytes, need);     // (launched on the second stream as well: that stream's scratch)
        return need;
    }
    void want_part_bf16(size_t need) { part_bytes = std::max(part_bytes, need); }
    // an error pass over lists writes one partial per wave
    void want_partials(int64_t n_out, int parts) { sq_elems = std::max(sq_elems, (size_t)(1 + srp_partials(n_out, parts))); }
};

// The E / D accumulators of all types form ONE contiguous range of the workspace, so that a relation-sharded run sums them
// over the ranks with a single all-reduce.  Three regions with the SAME internal layout -- all E, all D, all G (every type
// at the same offset in each) -- so that the distributed iteration can cut them into `world` equal element ranges:
// reduce-scatter of E and of D, update of the owned range of G, all-gather of G (skf_iterate_dist).  A pad behind each
// region takes the rounding of the last range.
static void layout_flat_regions(skf_plan* p) {
    const int n_types = (int)p->types.size();
    p->acc_off = p->ws_bytes;
    for (int region = 0; region < 3; ++region) {
        const size_t begin = p->ws_bytes;
        for (int i = 0; i < n_types; ++i) {
            TypeState& t = p->types[i];
            const bool active = (p->variant != SKF_TRANSFORM) || i == p->target;
            if (region < 2 && !active) continue;
            add_slot(p, region == 0 ? t.E : region == 1 ? t.D : t.G, (size_t)t.n_alloc * t.c * p->esz);
        }
        (region == 0 ? p->flat_e_off : region == 1 ? p->flat_d_off : p->flat_g_off) = begin;
        if (region == 0) p->flat_bytes = p->ws_bytes - begin;
        add_slot(p, p->flat_pad[region], 64 * 1024);
        if (region == 1) p->acc_bytes = p->ws_bytes - p->acc_off;
    }
    // the Gram matrices of all types form one range (SKF_OPT_OWNED_ROWS: one all-reduce of the partial sums)
    p->xg_off = p->ws_bytes;
    for (TypeState& t : p->types) add_slot(p, t.Gram, (size_t)t.c * t.c * 8);
    p->xg_bytes = p->ws_bytes - p->xg_off;
}

// what a type keeps beside G, E, D and Gram: its bf16 forms, the factor before the last update, the pseudo-inverse and the
// roundings of its B sums -- or, the target of a fold-in, its constant terms and the second factor buffer
static void layout_type(skf_plan* p, LayoutMax& m, int i) {
    TypeState& t = p->types[i];
    if (p->bf16) {
        t.ldgt = pad64(t.n);
        add_slot(p, t.GTb, (size_t)t.c * t.ldgt * 2);
    }
    m.gram_group += m.want_part(kind_gram(p), t.c, t.c, t.n, true);         // Gram = G^T G (gram_all: either stream)
    if (t.keep_prev) add_slot(p, t.Gp, (size_t)t.n * t.c * p->esz);
    if (p->bf16 && t.need_rows) {
        t.ldrow = (t.c + 7) / 8 * 8;
        add_slot(p, t.Grow, ((size_t)t.n_alloc + 1) * t.ldrow * 2);     // (+ 1: the all-zero row of the v6 list kernel)
    }
    if (p->variant != SKF_TRANSFORM) {
        add_slot(p, t.K, (size_t)t.c * t.c * 8);
        if (!p->f64) for (Slot* q : {&t.Bp32, &t.Bn32}) add_slot(p, *q, (size_t)t.c * t.c * 4);
        if (t.n_pad > m.maxn) m.maxn = t.n_pad;
    } else if (i == p->target) {
        for (Slot* q : {&t.Ec, &t.Dc, &t.Galt}) add_slot(p, *q, (size_t)t.n * t.c * p->esz);
        for (Slot* q : {&t.Bp_tot, &t.Bn_tot}) add_slot(p, *q, (size_t)t.c * t.c * 8);
    }
}

// SKF_DFMF / SKF_DFMC: the per-type sums of B+ / B- form one range (one memset per iteration clears them all); then the
// exchange ranges of row-block sharding: all W; the Q of unmasked, then of masked relations
static void layout_sums_and_exchange_ranges(skf_plan* p) {
    p->btot_off = p->ws_bytes;
    for (TypeState& t : p->types)
        for (Slot* q : {&t.Bp_tot, &t.Bn_tot}) add_slot(p, *q, (size_t)t.c * t.c * 8);
    p->btot_bytes = p->ws_bytes - p->btot_off;
    p->xw_off = p->ws_bytes;
    for (RelState& r : p->rels) add_slot(p, r.W, (size_t)p->types[r.row].c * p->types[r.col].c * 8);
    p->xw_bytes = p->ws_bytes - p->xw_off;
    for (const bool masked : {false, true}) {
        (masked ? p->xqm_off : p->xq_off) = p->ws_bytes;
        for (RelState& r : p->rels)
            if (r.masked == masked) add_slot(p, r.Q, (size_t)p->types[r.col].n_alloc * p->types[r.row].c * p->esz);
        (masked ? p->xqm_bytes : p->xq_bytes) = p->ws_bytes - (masked ? p->xqm_off : p->xq_off);
    }
}

// -- the groups the forms of a relation share --

// the c x c algebra of a relation (relation_small_terms; small_gemm: either stream): S Gram_j, Gram_i S, B = U S^T, D = S^T U
static void want_small_algebra(const skf_plan* p, LayoutMax& m, int ci, int cj) {
    const ProductKind k = kind_small(p);
    m.want_part(k, ci, cj, cj, true);
    m.want_part(k, ci, cj, ci, true);
    m.want_part(k, ci, ci, cj, true);
    m.want_part(k, cj, cj, ci, true);
}
// the Gram / cross-Gram pair of the error's trace term (skf_objective.inc: gram_of into Xi / Xj) over `ni` rows of the row type
static void add_trace_gram_pair(skf_plan* p, LayoutMax& m, RelState& r, int64_t ni) {
    const TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    add_slot(p, r.Xi, (size_t)ti.c * ti.c * 8);
    add_slot(p, r.Xj, (size_t)tj.c * tj.c * 8);
    m.want_part(kind_wide(p), ti.c, ti.c, ni);
    m.want_part(kind_wide(p), tj.c, tj.c, tj.n);
}
// the partial outputs of the parts of the lists (only with more than one part): the row-side product `wa` wide, Q c_i wide
static void add_parted_outputs(skf_plan* p, RelState& r, int wa) {
    if (r.kn_pc > 1) add_slot(p, r.Apart, (size_t)r.kn_pc * r.nr * wa * p->esz);
    if (r.kn_pr > 1) add_slot(p, r.Qpart, (size_t)r.kn_pr * p->types[r.col].n * p->types[r.row].c * p->esz);
}
// The row lists and the column lists of a relation kept as its entries, `pc` / `pr` parts each: pointers per (row, part) /
// (column, part), `cap` indices and values a side, the residuals beside the column values (known entries only), and the
// counters of the bind-time build (build_known_lists_t / _csr_t, skf_bind.inc)
static void add_list_slots(skf_plan* p, RelState& r, int64_t rows, int64_t cols, int pc, int pr, size_t cap, bool residuals) {
    add_slot(p, r.KrPtr, ((size_t)rows * pc + 1) * 8);
    add_slot(p, r.KrIdx, cap * 4);
    add_slot(p, r.KrVal, cap * p->esz);
    add_slot(p, r.KcPtr, ((size_t)cols * pr + 1) * 8);
    add_slot(p, r.KcIdx, cap * 4);
    add_slot(p, r.KcVal, cap * p->esz);
    if (residuals) add_slot(p, r.KcE, cap * p->esz);
    add_slot(p, r.KCnt, std::max((size_t)rows * pc, 2 * (size_t)cols * pr) * 4);
}
// -- one function per form --

// The lists of a fold-in relation as handed over and T = G_p S' (fold_prepare / fold_known_prepare, skf_stages.inc):
// ~ entries + n * c, never n_t * n_p.  Returns the partner's type.
static const TypeState& add_fold_lists(skf_plan* p, RelState& r) {
    const TypeState& tt = p->types[p->target];
    const TypeState& tp = p->types[r.row == p->target ? r.col : r.row];
    const size_t cap = (size_t)r.kn_cap;
    add_slot(p, r.KrPtr, ((size_t)tt.n + 1) * 8);
    add_slot(p, r.KrIdx, cap * 4);
    add_slot(p, r.KrVal, cap * p->esz);
    add_slot(p, r.Tm, (size_t)tp.n * tt.c * p->esz);
    return tp;
}

// REL_FOLD_KNOWN -- fold_known_prepare, fold_known_step, fold_known_err_pass (skf_stages.inc); sqerr_fold_known: stored =
// known: the unsplit B_r and the plan's one X = G_t B_r; the error is a pass over the lists alone
static void layout_fold_known(skf_plan* p, LayoutMax& m, RelState& r) {
    const TypeState& tt = p->types[p->target];
    const TypeState& tp = add_fold_lists(p, r);
    add_slot(p, r.Bf, (size_t)tt.c * tt.c * 8);
    if (!p->fold_x.bytes) add_slot(p, p->fold_x, (size_t)tt.n * tt.c * p->esz);
    want_small_algebra(p, m, p->types[r.row].c, p->types[r.col].c);
    m.want_part(kind_mixed(p), tp.n, tt.c, tp.c);                           // T = G_p S'
    m.want_part(kind_mixed(p), tt.n, tt.c, tt.c);                           // X = G_t B_r
    m.want_partials(tt.n, 1);                                               // fold_known_err_pass: at most as many waves
}

// REL_FOLD -- fold_prepare, fold_err_pass (skf_stages.inc); sqerr_fold: H and the c x c matrices of the error
static void layout_fold(skf_plan* p, LayoutMax& m, RelState& r) {
    const TypeState& tt = p->types[p->target];
    const TypeState& tp = add_fold_lists(p, r);
    add_slot(p, r.H, (size_t)tt.n * tp.c * p->esz);
    add_slot(p, r.T1, (size_t)p->types[r.row].c * p->types[r.col].c * 8);
    add_trace_gram_pair(p, m, r, p->types[r.row].n);                        // Gram matrices of the error's trace term
    want_small_algebra(p, m, p->types[r.row].c, p->types[r.col].c);
    m.want_part(kind_mixed(p), tp.n, tt.c, tp.c);                           // T = G_p S'
    m.want_part(kind_mixed(p), tt.n, tp.c, tt.c);                           // H = G_t S / G_t S^T
    m.want_partials(tt.n, 1);                                               // fold_err_pass
}

// What REL_DENSE, REL_KNOWN and REL_STORED share -- the relations an iteration contracts (contract_relation, backbone_step,
// skf_steps.inc): H and P (not the known-entry form: it keeps A instead), Q of a fold-in, the backbone's scratch, W.
// Returns whether the plan holds rows of the relation: the rest of a form is for those.
static bool layout_contracted(skf_plan* p, LayoutMax& m, RelState& r, RelForm form) {
    const TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    const size_t es = p->esz, cc = (size_t)ti.c * tj.c * 8;
    const bool transform = p->variant == SKF_TRANSFORM;
    if (r.nr > 0 && form != REL_KNOWN) add_slot(p, r.H, (size_t)r.nr * tj.c * es);
    if (r.nr > 0 && form != REL_KNOWN && (!transform || r.row == p->target)) add_slot(p, r.P, (size_t)r.nr * tj.c * es);
    if (transform && r.col == p->target) add_slot(p, r.Q, (size_t)tj.n * ti.c * es);
    if (!transform) {
        add_slot(p, r.T1, cc);
        if (!p->f64) add_slot(p, r.S32, cc / 2);
        if (r.nr > 0) m.want_part(kind_wide(p), ti.c, tj.c, r.nr);              // W = G_i^T P
        if (r.nr > 0) m.want_part(kind_wide(p), ti.c, tj.c, tj.n);            // W = (R^T G_i)^T G_j ; known entries: W = Y^T G_j
    }
    want_small_algebra(p, m, ti.c, tj.c);
    if (r.nr <= 0 && form == REL_KNOWN) add_slot(p, r.U2, cc);    // (owned rows, none of this relation's here: the dense part of Q
                                                                //  is still added on this process's rows of the column type)
    return r.nr > 0;
}

// REL_KNOWN -- known_prepare, known_row_pass, known_col_pass, known_finish (skf_stages.inc); sqerr_known: the known entries
// as row lists and column lists, the gathered vectors, the row-side product, c x c scratch
static void layout_known(skf_plan* p, LayoutMax& m, RelState& r) {
    const TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    const size_t es = p->esz, cc = (size_t)ti.c * tj.c * 8;
    r.ldmb = (tj.n + 127) / 128 * 16;
    if (!r.kn_csr) add_slot(p, r.Mb, (size_t)r.nr * r.ldmb);                  // (bind time only; CSR-fed: no mask at all)
    add_list_slots(p, r, r.nr, tj.n, r.kn_pc, r.kn_pr, (size_t)r.kn_cap, true);
    r.kn_ldf = p->bf16 ? (ti.c + 7) / 8 * 8 : ti.c;
    if (p->bf16) add_slot(p, r.FiB, ((size_t)tj.n + 1) * r.kn_ldf * 2);     // (+ 1: the all-zero row of the v6 list kernel;
                                                                            //  the row type's vectors: ti.Grow)
    add_slot(p, r.Tm, (size_t)tj.n * ti.c * es);
    add_slot(p, r.A, (size_t)r.nr * ti.c * es);
    add_parted_outputs(p, r, ti.c);
    add_slot(p, r.Sp, cc);
    add_slot(p, r.U2, cc);
    add_trace_gram_pair(p, m, r, r.nr);                                       // G_i'^T G_i, G_j^T G_j'
    add_slot(p, r.Bf, (size_t)ti.c * ti.c * 8);
    m.want_part(kind_mixed(p), tj.n, ti.c, tj.c);                           // T = G_j S^T ; Q += G_j (S^T Gram_i)
    m.want_part(kind_mixed(p), r.nr, ti.c, ti.c);                             // A += G_i (S Gram_j S^T)
    m.want_partials(tj.n, r.kn_pr);                                         // the error pass walks the column lists
}

// REL_STORED -- sparse_pass, fill_sums, fill_err_terms (skf_stages.inc); sqerr_stored: the stored entries as row lists and
// column lists with their values, the partial outputs of the parts, the c x c Gram matrices of the error's trace term:
// everything ~ entries or n * c, nothing ~ n_i * n_j
static void layout_stored(skf_plan* p, LayoutMax& m, RelState& r) {
    const TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    add_list_slots(p, r, r.nr, tj.n, r.kn_pc, r.kn_pr, (size_t)r.kn_cap, false);
    add_parted_outputs(p, r, tj.c);
    add_trace_gram_pair(p, m, r, r.nr);                                       // Gram matrices of the error's trace term
    m.want_part(kind_mixed(p), r.nr, tj.c, ti.c);                           // H = G_i S
    m.want_part(kind_mixed(p), r.nr, ti.c, tj.c);                           // side products
    m.want_part(kind_mixed(p), tj.n, tj.c, ti.c);
    if (r.fill) {
        // the fill vectors, the two weighted column sums and their slab partials, the row sums of bind:
        // (n_i + n_j) (element + 8) + (slabs_i c_i + slabs_j c_j + c_i + c_j) 8 bytes -- O(n_i + n_j + slabs c)
        add_slot(p, r.Fa, (size_t)r.nr * p->esz);
        add_slot(p, r.Fb, (size_t)tj.n * p->esz);
        add_slot(p, r.Ft, (size_t)tj.c * 8);
        add_slot(p, r.Fs, (size_t)ti.c * 8);
        add_slot(p, r.FpartP, (size_t)cdiv(tj.n, COLSUM_ROWS) * tj.c * 8);
        add_slot(p, r.FpartQ, (size_t)cdiv(r.nr, COLSUM_ROWS) * ti.c * 8);
        add_slot(p, r.Frow, (size_t)r.nr * 8);
    }
    m.want_partials(r.nr, r.kn_pc);                                           // the error pass walks the row lists
}

// -- REL_DENSE and its helpers --

// the mask: a working copy of the relation that the completion writes into (f64 / f32) and the packed bits
static void add_mask_slots(skf_plan* p, RelState& r) {
    const int64_t cols = p->types[r.col].n;
    if (!r.mask) return;
    if (!p->bf16) add_slot(p, r.Rw, (size_t)r.nr * cols * p->esz);
    r.ldmb = (cols + 127) / 128 * 16;               // bytes per packed mask row: whole 128-column tiles
    add_slot(p, r.Mb, (size_t)r.nr * r.ldmb);
}
// SKF_BF16, masked: known entries as compact per-tile lists, up to 1/8 of the relation (beyond that the completion blends
// through the mask): 4 bytes per entry = at most a quarter of the bf16 relation's bytes (build_tile_lists, skf_bind.inc)
static void add_tile_lists(skf_plan* p, RelState& r) {
    const int64_t cols = p->types[r.col].n;
    const size_t tiles = (size_t)cdiv(r.nr, 256) * cdiv(cols, 128);     // (128-column tiles: the finer grid)
    r.kcap = (size_t)r.nr * cols / 8 + 4096;
    add_slot(p, r.Kcnt, tiles * 4);
    add_slot(p, r.Koff, (tiles + 1) * 4);
    add_slot(p, r.Klist, r.kcap * 4);
}
// SKF_BF16, an unmasked 0/1 relation: room for the CSR / CSC form of a sparse one beside its bitmap (build_sparse_pattern,
// skf_bind.inc), in parts where the ones gather bf16 factor rows (ones_pass)
static void add_ones_lists(skf_plan* p, LayoutMax& m, RelState& r) {
    const TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    const int64_t per = r.sp_gather ? 80 : 256;            // (one entry in 80 / in 256 set, see build_sparse_pattern)
    r.sp_cap = (int64_t)r.nr * tj.n / per > 0 ? (int64_t)r.nr * tj.n / per : 1;
    if (r.sp_gather) {
        if (r.sp_pc > 1) add_slot(p, r.SpRpP, ((size_t)r.nr * r.sp_pc + 1) * 8);
        if (r.sp_pr > 1) add_slot(p, r.SpCpP, ((size_t)tj.n * r.sp_pr + 1) * 8);
        const size_t pb = std::max(r.sp_pc > 1 ? (size_t)r.sp_pc * r.nr * tj.c * 4 : (size_t)0,
                                   r.sp_pr > 1 ? (size_t)r.sp_pr * tj.n * ti.c * 4 : (size_t)0);
        if (pb > m.sp_part_bytes) m.sp_part_bytes = pb;
    }
    add_slot(p, r.SpRp, (size_t)(r.nr + 1) * 8);
    add_slot(p, r.SpCp, (size_t)(tj.n + 1) * 8);
    add_slot(p, r.SpCi, (size_t)r.sp_cap * 4);
    add_slot(p, r.SpRi, (size_t)r.sp_cap * 4);
    add_slot(p, r.SpCnt, (size_t)(r.nr + 2 * tj.n + 8) * 4);
}
// SKF_BF16: the operands of the completion / residual tiles, and the ONE stored copy of the relation -- padded bf16 or a bitmap
static void add_bf16_copies(skf_plan* p, LayoutMax& m, RelState& r) {
    const TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    r.ldhb = pad64(tj.c);
    add_slot(p, r.Hb, (size_t)r.nr * r.ldhb * 2);
    add_slot(p, r.Gb, (size_t)tj.n * r.ldhb * 2);
    r.ldrb = pad64(tj.n);
    r.kq = pad64(r.nr);
    if (r.binary) {
        r.ldbb = r.ldrb / 8;
        add_slot(p, r.Bb, (size_t)r.kq * r.ldbb);
        if (!r.masked) add_ones_lists(p, m, r);
    } else {
        add_slot(p, r.Rb, (size_t)r.kq * r.ldrb * 2);
    }
    m.want_part_bf16(bf16_part_bytes((int)r.nr, tj.c, (int)r.ldrb, r.binary));     // P = R G_j
    m.want_part_bf16(bf16_part_bytes((int)tj.n, ti.c, (int)r.kq, true));         // Q = R^T G_i
}

// REL_DENSE -- relation_gemm (skf_plan.inc), complete_relation, side_terms, launch_tile_epilogue (skf_steps.inc);
// sqerr_dense: the matrix itself in the caller's memory (f64 / f32 unmasked) or in one of the copies above
static void layout_dense(skf_plan* p, LayoutMax& m, RelState& r) {
    const TypeState &ti = p->types[r.row], &tj = p->types[r.col];
    add_mask_slots(p, r);
    if (p->bf16) {
        if (r.mask) add_tile_lists(p, r);
        add_bf16_copies(p, m, r);
    } else {
        m.want_part(kind_relation(p), r.nr, tj.c, tj.n);                      // P = R G_j
        m.want_part(kind_relation(p), tj.n, ti.c, r.nr);                      // Q = R^T G_i
        if (r.mask) m.want_part(kind_plan(p), r.nr, tj.n, tj.c);              // the completion H G_j^T
    }
    m.want_part(kind_mixed(p), r.nr, tj.c, ti.c);                           // H = G_i S
    m.want_part(kind_mixed(p), r.nr, ti.c, tj.c);                           // side products
    m.want_part(kind_mixed(p), tj.n, tj.c, ti.c);
    const size_t blocks = (size_t)cdiv(r.nr, 32) * cdiv(tj.n, 32);            // residual partials: smallest tile any engine uses
    if (blocks > m.sq_elems) m.sq_elems = blocks;
}

static void layout_relation(skf_plan* p, LayoutMax& m, RelState& r) {
    const size_t cc = (size_t)p->types[r.row].c * p->types[r.col].c * 8;
    if (p->variant == SKF_TRANSFORM) { r.nr = p->types[r.row].n; r.r0 = 0; }
    add_slot(p, r.S, cc);
    add_slot(p, r.U, cc);
    const RelForm form = form_of(r);
    switch (form) {
    case REL_FOLD_KNOWN: layout_fold_known(p, m, r); break;
    case REL_FOLD:       layout_fold(p, m, r); break;
    case REL_KNOWN:      if (layout_contracted(p, m, r, form)) layout_known(p, m, r); break;
    case REL_STORED:     if (layout_contracted(p, m, r, form)) layout_stored(p, m, r); break;
    case REL_DENSE:      if (layout_contracted(p, m, r, form)) layout_dense(p, m, r); break;
    }
}

// small graphs: every rank <= 64, sparse constraints only, a few thousand objects per type -> the fused schedule
static void plan_layout_small_graph(skf_plan* p) {
    const int n_types = (int)p->types.size(), n_relations = (int)p->rels.size(), n_thetas = (int)p->thetas.size();
    bool ok = p->variant == SKF_DFMF && p->engine == SKF_ENGINE_MFMA && !p->bf16 && !p->sliced && n_types <= SM_MAXT &&
              n_relations >= 1 && n_relations <= SM_MAXR && n_thetas <= SM_MAXTH;
    // (object counts: the Q shares of the schedule grow with n_i / 256 * n_j * c_i, and from a few thousand objects
    // on the relation contractions are worth the big tiles of the general schedule)
    for (const TypeState& t : p->types) ok = ok && t.c <= SMALLC && t.n <= SM_MAX_OBJECTS;
    // (a constraint given as its entries is kept as lists whatever its density; it rides this schedule under the documented
    // condition, 0 < nnz <= n * n / SKF_THETA_SPARSE_DIV, like the dense-fed form)
    for (const ThetaState& th : p->thetas)
        ok = ok && th.sparse && (!th.entries || (th.nnz_cap > 0 && th.nnz_cap <= p->types[th.type].n * p->types[th.type].n / SKF_THETA_SPARSE_DIV));
    // (dense relations only.  Under the terms above -- SKF_DFMF, hence no mask, no known entries and no fold-in -- that
    // says: not SKF_REL_SPARSE_CSR)
    for (const RelState& r : p->rels) ok = ok && !r.absent && !r.masked && form_of(r) == REL_DENSE;
    p->small_fused = ok;
    if (!ok) return;
    size_t wdoubles = 0, gdoubles = 0;
    for (size_t k = 0; k < p->rels.size(); ++k) {
        RelState& r = p->rels[k];
        const TypeState &ti = p->types[r.row], &tj = p->types[r.col];
        int part = 0;
        for (int64_t r0 = 0; r0 < ti.n; r0 += 64) p->sm_j1.push_back(SmJob{SMJ_P, (int)k, (int)r0, (int)std::min<int64_t>(64, ti.n - r0), part++, 0, 0, 0});
        // Q = R^T G_i: a long inner dimension (the rows of the relation) over a small output -> shares of SM_QROWS rows
        int qpart = 0;
        for (int64_t k0 = 0; k0 < ti.n; k0 += SM_QROWS, ++qpart)
            for (int64_t c0 = 0; c0 < tj.n; c0 += 64)
                p->sm_j1.push_back(SmJob{SMJ_Q, (int)k, (int)c0, (int)std::min<int64_t>(64, tj.n - c0), qpart, (int)k0,
                                         (int)std::min<int64_t>(SM_QROWS, ti.n - k0), 0});
        r.sm_qparts = qpart;
        wdoubles += align_up((size_t)part * ti.c * tj.c, 16);      // (shares of different relations / types never share a cache line)
        add_slot(p, r.SmQ, (size_t)qpart * tj.n * ti.c * p->esz);
        for (Slot* q : {&r.SmBp, &r.SmBn}) add_slot(p, *q, (size_t)ti.c * ti.c * 8);
        for (Slot* q : {&r.SmDp, &r.SmDn}) add_slot(p, *q, (size_t)tj.c * tj.c * 8);
    }
    for (size_t i = 0; i < p->types.size(); ++i) {
        const TypeState& t = p->types[i];
        int part = 0;
        for (int64_t r0 = 0; r0 < t.n; r0 += SM_GROWS) p->sm_j1.push_back(SmJob{SMJ_GRAM, (int)i, (int)r0, (int)std::min<int64_t>(SM_GROWS, t.n - r0), part++, 0, 0, 0});
        gdoubles += align_up((size_t)part * t.c * t.c, 16);
        for (int64_t r0 = 0; r0 < t.n; r0 += 64) p->sm_j3.push_back(SmJob{0, (int)i, (int)r0, (int)std::min<int64_t>(64, t.n - r0), 0, 0, 0, 0});
        bool constrained = false;
        for (const ThetaState& th : p->thetas) constrained = constrained || th.type == (int)i;
        if (constrained)      // one wave per row, four rows per workgroup
            for (int64_t r0 = 0; r0 < t.n; r0 += 4) p->sm_j1.push_back(SmJob{SMJ_THETA, (int)i, (int)r0, (int)std::min<int64_t>(4, t.n - r0), 0, 0, 0, 0});
    }
    // Gram shares first (the inverse hangs off the last of them), then P (W hangs off the last of those), Q, constraints
    auto prio = [](const SmJob& j) { return j.kind == SMJ_GRAM ? 0 : (j.kind == SMJ_P ? 1 : (j.kind == SMJ_Q ? 2 : 3)); };
    std::stable_sort(p->sm_j1.begin(), p->sm_j1.end(), [&](const SmJob& a, const SmJob& b) { return prio(a) < prio(b); });
    add_slot(p, p->sm_tables, sizeof(SmTables));
    add_slot(p, p->sm_jobs1, p->sm_j1.size() * sizeof(SmJob));
    add_slot(p, p->sm_jobs3, p->sm_j3.size() * sizeof(SmJob));
    add_slot(p, p->sm_wpart, wdoubles * 8);
    add_slot(p, p->sm_gpart, gdoubles * 8);
    add_slot(p, p->sm_tickets, (p->types.size() + p->rels.size()) * sizeof(int));
    add_slot(p, p->sm_batch, SKF_MAX_BATCH * sizeof(void*));          // table of tables: [0] = this plan's
}

// the constraints (theta_terms_rows, skf_plan.inc): the CSR form with its hub-row tables, or -- SKF_BF16 -- the bf16 halves
static void layout_constraints(skf_plan* p, LayoutMax& m) {
    for (ThetaState& th : p->thetas) {
        TypeState& t = p->types[th.type];
        if (th.sparse) {
            // (local rows: everything from the slice -- a scratch word for the validation, count + 1 pointers)
            add_slot(p, th.Cnt, th.local ? sizeof(int) : (size_t)t.n * sizeof(int));
            add_slot(p, th.Rp, (size_t)((th.local ? th.ln : t.n) + 1) * sizeof(int64_t));
            add_slot(p, th.Ci, (size_t)th.nnz_cap * sizeof(int));
            add_slot(p, th.Vv, (size_t)th.nnz_cap * p->esz);
            if (th.seg_cap > 0) {       // hub rows: segment table, row table, the e / d partials of every segment
                add_slot(p, th.HubSeg, (size_t)th.seg_cap * sizeof(ThetaSeg));
                add_slot(p, th.HubRows, (size_t)th.seg_cap * sizeof(ThetaHub));
                add_slot(p, th.HubE, (size_t)th.seg_cap * t.c * p->esz);
                add_slot(p, th.HubD, (size_t)th.seg_cap * t.c * p->esz);
            }
            continue;
        }
        if (!p->bf16) m.want_part(kind_plan(p), t.n, t.c, t.n);             // dense Theta G
        if (p->bf16) {
            th.ldb = pad64(t.n);
            add_slot(p, th.Pb, (size_t)t.n * th.ldb * 2);
            add_slot(p, th.Nb, (size_t)t.n * th.ldb * 2);
            m.want_part_bf16(bf16_part_bytes((int)t.n, t.c, (int)th.ldb, false));
            m.theta_tmp_bytes = std::max(m.theta_tmp_bytes, (size_t)t.n * t.c * 4);
        }
    }
    if (!p->thetas.empty()) add_slot(p, p->theta_flags, p->thetas.size() * 2 * sizeof(int));
    if (m.theta_tmp_bytes) add_slot(p, p->theta_tmp, m.theta_tmp_bytes);
}

// the scratch every launch shares, from the maxima gathered on the way
static void layout_shared_scratch(skf_plan* p, LayoutMax& m) {
    const size_t n_types = p->types.size();
    // the Gram products of all types side by side in one launch (gram_all): every product's slices at once
    if (n_types >= 2 && n_types <= 4) {
        m.part_bytes = std::max(m.part_bytes, m.gram_group);
        m.aux_bytes = std::max(m.aux_bytes, m.gram_group);
    }
    p->part_bytes = m.part_bytes;
    add_slot(p, p->part, m.part_bytes);
    if (m.sp_part_bytes) add_slot(p, p->sp_part, m.sp_part_bytes);
    p->part_aux_bytes = m.aux_bytes;
    add_slot(p, p->part_aux, m.aux_bytes);
    p->sq_elems = m.sq_elems;
    add_slot(p, p->sqpart, m.sq_elems * 8);
}

// the batched pseudo-inverse (skf_pinv.inc): every type's matrix at the largest eigen order
static void layout_eigen_scratch(skf_plan* p, int maxn) {
    const int n_types = (int)p->types.size();
    p->eig_maxn = maxn;
    p->eig_stride = (int64_t)maxn * maxn;
    const size_t mat = (size_t)p->eig_stride * n_types * sizeof(double);
    for (Slot* q : {&p->eigA, &p->eigV, &p->eigVs}) add_slot(p, *q, mat);
    add_slot(p, p->eigW, (size_t)maxn * n_types * sizeof(double));
    for (Slot* q : {&p->eigN, &p->eigNorig, &p->eigOk}) add_slot(p, *q, (size_t)n_types * sizeof(int));
    if (maxn > SWEEP_MAXN && n_types <= PINV_MAXB) add_slot(p, p->eigX, defl_scratch_bytes(n_types, p->eig_stride));
}

static void plan_layout(skf_plan* p) {
    const bool fit = p->variant != SKF_TRANSFORM;
    LayoutMax m{p};
    layout_flat_regions(p);         // ... and the Gram range
    for (int i = 0; i < (int)p->types.size(); ++i) layout_type(p, m, i);
    if (fit) layout_sums_and_exchange_ranges(p);
    for (RelState& r : p->rels) layout_relation(p, m, r);
    plan_layout_small_graph(p);
    layout_constraints(p, m);
    layout_shared_scratch(p, m);
    if (fit) layout_eigen_scratch(p, m.maxn);
}
