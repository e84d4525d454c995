// skf_plan.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): the plan -- its switches, the state of a type / a relation / a constraint, the form a relation comes
// in (RelForm), the workspace slots -- and the launch primitives the steps are put together from: the product kinds and
// their split-K scratch, the relation contractions, Gram, the constraint terms, the c x c terms, the fused side update.
// Plan creation: skf_create.inc; the steps of an iteration: skf_steps.inc; the pseudo-inverse: skf_pinv.inc.
// ------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------
// Test / A-B switches from the environment.  A plan reads them ONCE, when its workspace is bound (skf::Switches::read);
// no launch path reads the environment.  Defaults are the measured best (DESIGN.md section 10).
struct Switches {
    bool pinv_jacobi = false;      // SKF_PINV_JACOBI=1     every pseudo-inverse through the Jacobi eigen-solver
    bool chol_unblocked = false;   // SKF_CHOL_UNBLOCKED=1  plain (unblocked) Cholesky inverse
    bool chol_no_small = false;    // SKF_CHOL_NO_SMALL=1   no one-wave kernel for orders <= 64
    bool no_small_chain = false;   // SKF_NO_SMALL_CHAIN=1  general c x c launches instead of the one-workgroup chains
    bool debug_pinv = false;       // SKF_DEBUG_PINV=1      per iteration: verdict of the fast path (stderr; synchronises)
    bool graph = false;            // SKF_GRAPH=1           hipGraph replay of the iteration
    bool no_overlap = false;       // SKF_NO_OVERLAP=1      no second stream
    bool no_pipeline = false;      // SKF_NO_PIPELINE=1     staged schedule instead of the relation pipeline
    int side_tile = 0;             // SKF_SIDE_TILE=64|128  tile shape of the fused side update
    bool no_small_fused = false;   // SKF_NO_SMALL_FUSED=1  small graphs on the general staged schedule (~33 launches per iteration)
    bool no_sweep = false;         // SKF_PINV_SWEEP=0      orders 65 .. 256: blocked Cholesky inverse + unpack instead of the blocked sweep (A/B)
    bool small_sweep1 = false;     // SKF_SMALL_SWEEP4=0    small graphs: one pivot per barrier in the register sweep (same bits; A/B, tests)
    int gram_sym = 1;              // SKF_GRAM_SYM=0        split-K Gram products compute every tile (default: the tiles on / below the diagonal, mirrored by the reduce)
    bool gram_group = true;        // SKF_GRAM_GROUP=0      the Gram products of the types as launches of their own (default: one grouped launch + one reduce; same bits)
    int sweep_step_min = 65;       // SKF_SWEEP_STEP_MIN=n  orders >= n take the blocked sweep one launch per block step with the update of a step
                                   //                       spread over row slabs (sweep_step_kernel); below: one workgroup per matrix, one launch.
                                   //                       0 = never (A/B; same bits either way)
    int sweep_rows = 32;           // SKF_SWEEP_ROWS=32|64.. rows of a slab (a multiple of 32)
    bool no_pairs = false;         // SKF_CHAIN_PAIRS=0     the independent c x c products of a relation's chain as launches of their own (A/B; same bits)
    bool no_sweep_big = false;     // SKF_SWEEP_BIG=0       orders above 256 on the blocked Cholesky inverse + unpack, as before round 5 (A/B)
    int dfmc_sparse = -1;          // SKF_DFMC_SPARSE=0|1   masked relations never / whenever a bound is given as lists of their known entries
    int known_parts = 0;           // SKF_KNOWN_PARTS=1|2|4|8  parts of the known-entry lists (0: by the size of the gathered matrix)
    bool known_parts_forced = false;   // ... given at all: short lists are cut into parts too (tests)
    bool comm_stream = true;       // SKF_COMM_STREAM=0     plans with owned rows: the exchanges on the main stream (A/B; tests run both)
    bool early_update = true;      // SKF_EARLY_UPDATE=0    pipeline: every type is updated at the end of the iteration (default: a type whose last relation is through
                                   //                       and that nothing reads any more is updated on the second stream, underneath the remaining contractions)
    int theta_hub_row = THETA_HUB_ROW;   // SKF_THETA_HUB_ROW=n   rows of a sparse constraint longer than n entries are cut into segments of n, a wave
                                   //                       each (theta_hub_partial_kernel / _combine_kernel); 0 = never.  Read when the plan
                                   //                       is CREATED (the partial-sum scratch is sized from it), as SKF_DFMC_SPARSE is
    static Switches read() {
        auto on = [](const char* name) { return env_int(name, 0) != 0; };
        auto off = [](const char* name) { return env_int(name, 1) == 0; };         // "=0" switches a default off
        Switches w;
        w.pinv_jacobi = on("SKF_PINV_JACOBI");
        w.chol_unblocked = on("SKF_CHOL_UNBLOCKED");
        w.chol_no_small = on("SKF_CHOL_NO_SMALL");
        w.no_small_chain = on("SKF_NO_SMALL_CHAIN");
        w.debug_pinv = on("SKF_DEBUG_PINV");
        w.graph = on("SKF_GRAPH");
        w.no_overlap = on("SKF_NO_OVERLAP");
        w.no_pipeline = on("SKF_NO_PIPELINE");
        w.no_small_fused = on("SKF_NO_SMALL_FUSED");
        w.no_sweep = off("SKF_PINV_SWEEP");
        w.small_sweep1 = off("SKF_SMALL_SWEEP4");
        w.gram_sym = off("SKF_GRAM_SYM") ? 0 : 1;
        w.early_update = !off("SKF_EARLY_UPDATE");
        w.gram_group = !off("SKF_GRAM_GROUP");
        w.sweep_step_min = env_int("SKF_SWEEP_STEP_MIN", w.sweep_step_min);
        { const int sr = env_int("SKF_SWEEP_ROWS", 0); if (sr >= 32) w.sweep_rows = (sr + 31) / 32 * 32; }
        w.no_sweep_big = off("SKF_SWEEP_BIG");
        w.no_pairs = off("SKF_CHAIN_PAIRS");
        w.side_tile = env_int("SKF_SIDE_TILE", 0);
        w.dfmc_sparse = env_int("SKF_DFMC_SPARSE", -1);
        { const int kp = env_int("SKF_KNOWN_PARTS", 0); w.known_parts = (kp == 1 || kp == 2 || kp == 4 || kp == 8) ? kp : 0; }
        w.known_parts_forced = env_str("SKF_KNOWN_PARTS") != nullptr;
        w.comm_stream = !off("SKF_COMM_STREAM");
        { const int hr = env_int("SKF_THETA_HUB_ROW", THETA_HUB_ROW); w.theta_hub_row = hr > 0 ? hr : 0; }
        return w;
    }
};

struct Slot {            // a workspace sub-allocation
    size_t off = 0, bytes = 0;
    void* ptr = nullptr;
};

struct TypeState {
    int64_t n = 0;
    int c = 0;
    int n_pad = 0;                 // eigen order (even)
    Slot G, E, D, Gram, K;
    Slot Bp32, Bn32;               // f32 engines: roundings of Bp_tot / Bn_tot for the fused side update
    Slot Bp_tot, Bn_tot;           // sum over the relations of the B / D matrices' + and - parts (c x c f64)
    Slot Ec, Dc;                   // SKF_TRANSFORM target only
    Slot Galt;                     // SKF_TRANSFORM target: the second factor buffer of the one-launch iteration (foldin_step_kernel)
    int64_t t0 = 0, tn = 0;        // rows whose type-level terms G (sum B) this plan adds (row-block sharding)
    // SKF_OPT_OWNED_ROWS: [t0, t0 + tn) are the rows this plan OWNS; `chunk` rows per rank in the padded layout of the
    // exchanges (G, E, D, the bf16 rows and every Q over this type hold part_count * chunk rows)
    int64_t chunk = 0, n_alloc = 0;
    bool gather_master = true;     // the all-gather of the updated rows carries the master copy (false: SKF_BF16 operand rows only)
    Slot GTb;                      // SKF_BF16: bf16 transpose of G, [c][pad64(n)], zero padded
    int64_t ldgt = 0;
    bool set = false;
    bool keep_prev = false;        // a known-entries relation touches this type: Gp = the factor before the last update
    Slot Gp;
    // SKF_BF16: the bf16 ROWS of G, [n + 1][ldrow] with an all-zero last row -- the gathered matrix of the list passes over
    // the known entries of a masked relation and over the ones of a sparse 0/1 relation (skf_known.h); kept in step with GTb
    bool need_rows = false;
    Slot Grow;
    int64_t ldrow = 0;
};

struct RelState {
    int row = 0, col = 0;
    const void* R_in = nullptr;
    int64_t ld_in = 0;
    const uint8_t* mask = nullptr;
    int64_t ldmask = 0;
    const void* R = nullptr;       // matrix the iteration reads (R_in or the DFMC working copy)
    int64_t ldr = 0;
    Slot Rw, P, Q, W, T1, S, U, H;
    Slot S32;                      // f32 engines: rounding of S for the fused side update
    Slot Hb, Gb;                   // SKF_BF16: bf16 H = G_i S and bf16 G_j (K padded to 64) for the completion / residual tiles
    int64_t ldhb = 0;
    Slot Rb;                       // SKF_BF16: the ONE stored copy of the relation, bf16 [pad64(nr)][pad64(n_j)], zero padded
    int64_t ldrb = 0;
    int64_t kq = 0;                // pad64(nr): inner dimension of Q = R^T G_i (padding rows of Rb are zero)
    bool binary = false;           // SKF_BF16 + SKF_REL_BINARY: the relation is stored as a bitmap (Bb) instead of Rb
    Slot Bb;                       // bitmap [pad64(nr)][ldbb bytes], bit (c & 7) of byte c >> 3; padding zero
    int64_t ldbb = 0;
    // a very sparse binary relation (at most 1 entry in 256 set): the positions of the ones as CSR and CSC beside the bitmap
    bool sparse = false;
    Slot SpRp, SpCi, SpCp, SpRi, SpCnt;     // row pointers / columns, column pointers / rows (ascending), count scratch
    int64_t sp_cap = 0, sp_nnz = 0;
    // ... contracted by srp_bf16_v6_kernel<.., SRP_ONES> over bf16 factor rows when both ranks are 64 / 128 / 256 (up to 1
    // entry in 80 set); otherwise by binary_spmm_kernel over the f32 rows (up to 1 in 256).  Lists in parts pinned to XCDs:
    bool sp_gather = false;
    int sp_pc = 1, sp_pr = 1;               // column parts of the row lists (P), row parts of the column lists (Q)
    int64_t sp_pw = 0, sp_ph = 0;
    Slot SpRpP, SpCpP;                      // segment pointers of the parted lists
    Slot Mb;                       // DFMC: the mask as packed bits, [nr][ldmb bytes], bit (n & 7) of byte n >> 3
    int64_t ldmb = 0;
    bool mask_is_bits = false;     // the caller's mask is already packed (SKF_REL_MASK_BITS)
    Slot Kcnt, Koff, Klist;        // SKF_BF16 masked relation: known entries per 256 x 256 tile (counts, offsets, entries)
    size_t kcap = 0;               // capacity of Klist in entries
    bool use_klist = false;        // the lists fit: the completion writes whole tiles and never reads R back
    bool s_set = false;
    // row-block sharding: this plan holds rows [r0, r0 + nr) of the relation (nr == n_i: all of it)
    int64_t r0 = 0, nr = 0;
    bool absent = false;           // no local rows (W, Q, S are still kept for the exchange)
    bool masked = false;           // DFMC: the relation has a mask (here or, for an absent one, elsewhere)
    bool col_side = true;          // this plan adds the column-side terms E_j, D_j
    // DFMC on the known entries only (skf_relation_desc.known_bound, skf_known.h): no completed copy of the relation
    bool kn = false;
    int64_t kn_cap = 0, kn_nnz = 0;        // bound given at plan creation / entries found at bind time
    int kn_pc = 1, kn_pr = 1;              // column parts of the row lists, row parts of the column lists
    int64_t kn_pw = 0, kn_ph = 0;          // columns per column part (multiple of 64), rows per row part
    int64_t kn_ldf = 0;                    // leading dimension of the gathered vectors (bf16 copies: padded to 8)
    Slot KrPtr, KrIdx, KrVal;              // rows -> known columns (ascending), R there
    Slot KcPtr, KcIdx, KcVal, KcE;         // columns -> known rows (ascending), R there, residuals E of the last iteration
    Slot KCnt;                             // count / fill-position scratch of the bind-time build
    bool kn_csr = false;                   // SKF_REL_KNOWN_CSR: the lists come from the caller's CSR, not from a mask
    const int64_t* csr_ptr = nullptr;      // the caller's CSR (skf_plan_set_known_entries; read at bind time only)
    const int* csr_idx = nullptr;
    const void* csr_val = nullptr;
    // SKF_REL_SPARSE_CSR: the relation is the CSR of its stored entries, every other entry ZERO (DFMF, unmasked DFMC relations).
    // Row lists KrPtr / KrIdx / KrVal and column lists KcPtr / KcIdx / KcVal as above (parts kn_pc / kn_pr, values in the master
    // type), built at bind time from the caller's CSR; P = R G_j and Q = R^T G_i are SRP_APPLY passes over them with the stored
    // values where the known-entry form keeps residuals (sparse_pass), partial outputs of the parts in Apart / Qpart; the error
    // is tr(S^T Gram_i S Gram_j) (Xi, Xj) + one SRP_ERR pass with e = r.  No dense copy in any type.
    bool sp0 = false;
    // SKF_REL_FILL_RANK1 (with sp0): the relation is F = a b^T + D -- a filled relation with missing values.  The caller's
    // values are the true stored ones; bind turns the lists' values into d = v - a_r b_c (Fa / Fb: copies of a and b in the
    // master type).  sparse_pass adds a (b^T G_j) to P and b (a^T G_i) to Q: the weighted column sums Ft (c_j) / Fs (c_i) in
    // f64 from the slab partials FpartP / FpartQ (P and Q each their own: the relation pipeline runs on two streams).
    // fill_aa = |a|^2, fill_bb = |b|^2, fill_dab = 2 sum d a_r b_c: the constants of the error formula, f64, fixed order.
    bool fill = false;
    const void* fill_row = nullptr;        // the caller's a / b (skf_plan_set_relation_fill; read at bind time only)
    const void* fill_col = nullptr;
    Slot Fa, Fb, Ft, Fs, FpartP, FpartQ, Frow;
    double fill_aa = 0.0, fill_bb = 0.0, fill_dab = 0.0;
    // SKF_REL_FOLD_CSR (SKF_TRANSFORM): the new relation as ONE set of lists compressed along the target's side, copied into
    // KrPtr / KrIdx / KrVal at bind time (master type); Tm = G_p S^T (row side) / G_p S (column side), n_partner x c_target;
    // H = G_t S / G_t S^T (n_target x c_partner) and Xi / Xj / T1 for skf_relation_sqerr.  No P, no Q, no parts.
    bool fold = false;
    // ... with SKF_REL_FOLD_KNOWN: stored = KNOWN, every other entry takes the model's prediction in every iteration.  The same
    // lists and Tm; Bf = the UNSPLIT B_r = T^T T (c_t x c_t, f64) for X = G_t B_r of an iteration (skf_plan::fold_x); no H, no
    // trace term: skf_relation_sqerr is one pass over the lists (fold_known_kernel)
    bool fold_known = false;
    Slot FiB;                              // SKF_BF16: bf16 rows of T = G_j S^T (n_j x ldf; the rows of G_i: TypeState::Grow)
    Slot Tm;                               // T = G_j S^T in the master type (n_j x c_i)
    Slot Apart, Qpart;                     // partial outputs of the parts, [parts][n][c_i] (only with more than one part)
    Slot A;                                // E T, then the row-side product P S^T = G_i (S Gram_j S^T) + E T   (n_i x c_i)
    Slot Sp, Xi, Xj, Bf, U2;               // S of the stored residuals; G_i'^T G_i, G_j^T G_j'; S Gram_j S^T; S^T Gram_i  (f64)
    Slot SmBp, SmBn, SmDp, SmDn;           // small graphs: +- parts of S Gram_j S^T and S^T Gram_i S of THIS relation
    Slot SmQ;                              // ... and Q as shares over row ranges of the relation, [sm_qparts][n_j][c_i]
    int sm_qparts = 0;
};

// The form a relation comes in -- what the plan stores of it and which passes read it.  Every relation has exactly ONE; the
// flags above that decide it exclude each other (plan_describe_relation refuses every other combination, plan_decide_lists
// sets `kn` only where neither `sp0` nor `fold` is set):
//   REL_FOLD_KNOWN  fold && fold_known    SKF_TRANSFORM: the known entries along the target, everything else unknown
//   REL_FOLD        fold && !fold_known   SKF_TRANSFORM: the stored entries along the target, everything else zero
//   REL_STORED      sp0                   the stored entries as row and column lists, everything else zero (fill: + a b^T)
//   REL_KNOWN       kn                    SKF_DFMC: the known entries as row and column lists (kn_csr: from the caller's
//                                         CSR, else from a mask whose known share is small enough)
//   REL_DENSE       none of these         a matrix: f64 / f32, the padded bf16 copy or the bitmap (binary; sparse /
//                                         sp_gather: lists of its ones beside it), with or without a mask (masked)
// `absent` (no local rows) and `masked` go with REL_DENSE, REL_KNOWN and REL_STORED alike and change nothing about the form.
// `fold`, `fold_known` and `sp0` are final once the relation is described; `kn` is decided by plan_decide_lists, which reads
// REL_DENSE until then as "a matrix, or known entries that may yet become lists".  Everything after plan creation sees the final form.
enum RelForm { REL_DENSE, REL_KNOWN, REL_STORED, REL_FOLD, REL_FOLD_KNOWN };
static inline RelForm form_of(const RelState& r) {
    if (r.fold) return r.fold_known ? REL_FOLD_KNOWN : REL_FOLD;
    if (r.sp0) return REL_STORED;
    return r.kn ? REL_KNOWN : REL_DENSE;
}

struct ThetaState {
    int type = 0;
    const void* data = nullptr;
    int64_t ld = 0;
    bool has_pos = true, has_neg = true;   // non-empty halves of the +- split (found at bind time)
    Slot Pb, Nb;                           // SKF_BF16: bf16 copies of Theta+ / Theta-, [n][pad64(n)]
    int64_t ldb = 0;
    // sparse form (skf_theta_desc.nnz > 0): CSR in the master type, built at bind time
    bool sparse = false;
    int64_t nnz_cap = 0, nnz = 0;
    Slot Rp, Ci, Vv, Cnt;                  // rowptr (n + 1, int64), column indices (int32), values, per-row counts
    // skf_theta_desc.data == NULL: the CSR comes from the caller (skf_plan_set_constraint_entries; read at bind time only),
    // nnz_cap is its exact length and no dense form exists in any type -- kept as lists whatever the density
    bool entries = false;
    // ... and SKF_OPT_THETA_OWNED_ROWS: the caller's CSR is the slice of the OWNED rows [l0, l0 + ln) of the type over all
    // columns ("local rows"): Rp holds ln + 1 pointers from 0, Ci / Vv the slice, the hub tables carry LOCAL rows
    bool local = false;
    int64_t l0 = 0, ln = 0;
    // hub rows (longer than hub_row entries; 0: never split) cut into segments: the table and the rows it covers, sorted by
    // row, then by position; partial sums e / d per segment in HubE / HubD [n_seg][c], master type.  Host copies of the
    // rows and of their first segments: plans with owned rows launch the sub-range inside [t0, t0 + tn)
    int64_t hub_row = 0, seg_cap = 0, n_seg = 0;
    Slot HubSeg, HubRows, HubE, HubD;
    std::vector<int> hub_rows, hub_first;
    const int64_t* csr_ptr = nullptr;
    const int* csr_idx = nullptr;
    const void* csr_val = nullptr;
};

// Held-out pairs scored inside the fit (skf_plan_set_heldout; kernels skf_heldout.h, host side skf_heldout.inc): the lists
// the caller attached and where the monitor's own workspace keeps what belongs to them.  Empty `lists`: the plan is unmonitored.
struct HeldoutList {
    int rel = 0;
    int64_t n = 0;
    const int* rows = nullptr;
    const int* cols = nullptr;
    const void* vals = nullptr;
    int64_t blocks = 0;                    // slabs of the pass = f64 partials of the list
    void* H = nullptr;                     // G_i S (n_i x c_j, master type)
    void* part = nullptr;                  // split-K scratch of that product
    size_t part_bytes = 0;
};
struct HeldoutMonitor {
    std::vector<HeldoutList> lists;
    int patience = 0;
    double min_delta = 0.0;
    int64_t capacity = 0;
    HeldoutState* state = nullptr;         // device: the monitor's words
    int64_t* offs = nullptr;               // device: first partial of every list, n_lists + 1
    double* cur = nullptr;                 // device: the totals of the last evaluation, one per list
    double* partials = nullptr;
    double* history = nullptr;             // device: [capacity][n_lists]
    HeldoutSeg* segs = nullptr;            // device: the ranges the snapshot copies
    int n_segs = 0;
    int64_t max_words = 0;                 // longest range (the snapshot's grid)
    std::vector<void*> snap_g, snap_s;     // device: the best factor of every type / backbone of every relation
    std::vector<int64_t> host_offs;        // what `offs` / `segs` were uploaded from
    std::vector<HeldoutSeg> host_segs;
};

}  // namespace skf

struct skf_plan {
    int dtype = SKF_F32, variant = SKF_DFMF, target = -1, engine = SKF_ENGINE_MFMA;
    bool f64 = false, bf16 = false;
    size_t esz = 4;            // bytes of a master element (factors, E, D, P, Q, relations)
    int mt = SKF_F32;          // master type code; the c x c algebra is always SKF_F64
    std::vector<skf::TypeState> types;
    std::vector<skf::RelState> rels;
    std::vector<skf::ThetaState> thetas;
    std::vector<skf::Slot*> slots;
    size_t ws_bytes = 0;
    bool bound = false, prepared = false, first_iter = true;
    // shared scratch
    skf::Slot part;            // split-K partials
    size_t part_bytes = 0;
    skf::Slot eigA, eigV, eigVs, eigW, eigN, eigNorig, eigOk, sqpart;
    skf::Slot eigX;                        // scratch of the multi-workgroup deflation (plans with a rank above 256)
    skf::Slot theta_flags, theta_tmp;      // sign flags of the constraints; SKF_BF16: n x c product scratch
    int64_t eig_stride = 0;
    int eig_maxn = 0;
    size_t sq_elems = 0;
    // second stream: Gram + pseudo-inverse run concurrently with the relation contractions
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    skf::Slot part_aux;
    size_t part_aux_bytes = 0;
    skf::Slot sp_part;                     // partial outputs of the parted list passes over sparse 0/1 relations
    skf::Slot fold_x;                      // SKF_TRANSFORM with a SKF_REL_FOLD_KNOWN relation: X = G_t B_r of one relation, n_t x c_t

    skf::Switches sw;                      // read once in skf_plan_bind_workspace
    bool overlap = false;
    bool pipeline = true;                  // relation-pipelined schedule of the DFMF iteration (SKF_NO_PIPELINE=1 at bind: off)
    std::vector<hipEvent_t> ev_rel;        // one event per relation: its contractions are done
    size_t acc_off = 0, acc_bytes = 0;     // contiguous range of all E / D accumulators
    // E, D and G of all types as three regions of identical layout (flat_bytes each, a pad behind every one)
    size_t flat_e_off = 0, flat_d_off = 0, flat_g_off = 0, flat_bytes = 0;
    skf::Slot flat_pad[3];
    bool theta_owned = false;              // SKF_OPT_THETA_OWNED_ROWS: constraints given as their entries are slices of the owned rows
    skf_comm* comm = nullptr;              // collectives of the distributed iteration (skf_plan_set_comm; not owned)
    // SKF_OPT_OWNED_ROWS: ownership-aligned row blocks (iterate_owned)
    bool owned = false;
    int part_index = 0, part_count = 0;
    size_t xg_off = 0, xg_bytes = 0;       // contiguous range of every type's Gram matrix (one all-reduce of the partial sums)
    hipStream_t cs = nullptr;              // the stream the exchanges go out on
    std::vector<hipEvent_t> ev_own;
    bool masters_stale = false;            // SKF_BF16: rows of other owners hold old f32 values until finalize_owned
    // row-block sharding: contiguous ranges of all W, of the Q of unmasked / of masked relations
    bool sliced = false;
    size_t xw_off = 0, xw_bytes = 0, xq_off = 0, xq_bytes = 0, xqm_off = 0, xqm_bytes = 0;
    size_t btot_off = 0, btot_bytes = 0;   // contiguous range of every type's Bp_tot / Bn_tot
    void* ws_base = nullptr;
    // one captured iteration (hipGraph) for launch-bound graphs; replayed by skf_iterate
    hipGraphExec_t graph_exec = nullptr;
    hipStream_t graph_stream = nullptr;
    bool graph_failed = false;
    bool graph_on = false;                 // skf_plan_set_graph
    // optional hipEvent timing of the relation contractions (skf_plan_set_profiling)
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    double prof_flops = 0.0, prof_bytes = 0.0;
    int64_t prof_launches = 0;
    bool kn_first = true;                  // no residuals stored yet: E = the known entries themselves, S_prev = 0
    // small graphs (skf_small.h): the whole DFMF iteration as eight launches over job tables kept in the workspace
    bool small_fused = false;
    skf::Slot sm_tables, sm_jobs1, sm_jobs3, sm_wpart, sm_gpart, sm_tickets, sm_batch;
    std::vector<const void*> sm_batch_host;        // device addresses of the tables of the plans of the last batch (this plan first)
    std::vector<skf::SmJob> sm_j1, sm_j3;
    skf::HeldoutMonitor mon;               // skf_plan_set_heldout: held-out lists scored after every iteration of skf_iterate
    ~skf_plan() {
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_rel) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_own) (void)hipEventDestroy(e);
        if (cs) (void)hipStreamDestroy(cs);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (aux) (void)hipStreamDestroy(aux);
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    }
};

namespace skf {

static void add_slot(skf_plan* p, Slot& s, size_t bytes) {
    s.bytes = bytes;
    s.off = p->ws_bytes;
    p->ws_bytes += align_up(bytes ? bytes : 1, 256);
    p->slots.push_back(&s);
}

static hipStream_t as_stream(void* s) { return (hipStream_t)s; }

static void copy2d(void* dst, int64_t ldd, const void* src, int64_t lds, int64_t rows, int64_t cols,
                   size_t esz, hipStream_t st) {
    if (rows <= 0 || cols <= 0) return;
    SKF_HIP(hipMemcpy2DAsync(dst, (size_t)ldd * esz, src, (size_t)lds * esz, (size_t)cols * esz, (size_t)rows,
                             hipMemcpyDeviceToDevice, st));
}

static GemmArgs gemm_args(const void* A, int64_t sa_m, int64_t sa_k, const void* B, int64_t sb_k, int64_t sb_n,
                          void* C, int64_t ldc, int M, int N, int K, int epi, int nan) {
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = A; g.B = B; g.C = C; g.C2 = nullptr; g.mask = nullptr; g.part = nullptr;
    g.sa_m = sa_m; g.sa_k = sa_k; g.sb_k = sb_k; g.sb_n = sb_n;
    g.ldc = ldc; g.ldc2 = ldc; g.ldmask = 0;
    g.M = M; g.N = N; g.K = K; g.k_chunk = K;
    g.aop = AOP_NONE; g.epi = epi; g.nan_to_num = nan;
    return g;
}

// The product kinds of a plan: operand / result types and the relation / symmetric flags of their launches.  The launches below
// and the scratch sizing of skf_plan_create (kind_part_bytes) take them from here, so the two cannot drift apart.
struct ProductKind { GemmTypes ty; bool relation, sym; };
// master x master -> master: dense Theta, the reconstruction H G_j^T
static ProductKind kind_plan(const skf_plan* p) { return {{p->mt, p->mt, p->mt}, false, false}; }
// the same streaming a relation matrix (f32 / f64 engines): P = R G_j, Q = R^T G_i
static ProductKind kind_relation(const skf_plan* p) { return {{p->mt, p->mt, p->mt}, true, false}; }
// c x c algebra: f64 x f64 -> f64
static ProductKind kind_small(const skf_plan*) { return {{SKF_F64, SKF_F64, SKF_F64}, false, false}; }
// master x master -> f64 (W = G_i^T P, cross-Gram: long f64 accumulation over the object dimension) ...
static ProductKind kind_wide(const skf_plan* p) { return {{SKF_F64, p->mt, p->mt}, false, false}; }
// ... and Gram = G^T G, symmetric (where SKF_GRAM_SYM leaves it on: fewer tiles never ask for fewer slices, so sizing with it covers both)
static ProductKind kind_gram(const skf_plan* p) { return {{SKF_F64, p->mt, p->mt}, false, true}; }
// master x f64 -> master (n x c x c products with an f64 backbone / B / D matrix: H = G_i S, the side products)
static ProductKind kind_mixed(const skf_plan* p) { return {{p->mt, p->mt, SKF_F64}, false, false}; }
// split-K scratch a launch of kind `k` with these sizes can ask for
static size_t kind_part_bytes(const skf_plan* p, const ProductKind& k, int64_t M, int64_t N, int64_t K) {
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.M = (int)M; g.N = (int)N; g.K = (int)K; g.epi = EPI_STORE; g.sym = k.sym;
    return gemm_part_elems(k.ty, p->engine, g, k.relation) * (k.ty.c == SKF_F64 ? 8 : 4);
}
// A launch on the second stream takes that stream's split-K scratch (the main stream's partials may be in flight in `part`)
static void kind_gemm(skf_plan* p, const ProductKind& k, const GemmArgs& g, hipStream_t st, bool on_aux = false) {
    run_gemm(k.ty, p->engine, g, 0, on_aux ? p->part_aux.ptr : p->part.ptr, on_aux ? p->part_aux_bytes : p->part_bytes, st, k.relation);
}
static void plan_gemm(skf_plan* p, GemmArgs g, hipStream_t st) { kind_gemm(p, kind_plan(p), g, st); }
// (c x c algebra on the second stream: ranks above 512 leave the deep unsplit tile and are cut into K slices)
static void small_gemm(skf_plan* p, GemmArgs g, hipStream_t st) { kind_gemm(p, kind_small(p), g, st, p->aux != nullptr && st == p->aux); }
static void wide_gemm(skf_plan* p, GemmArgs g, hipStream_t st) { kind_gemm(p, kind_wide(p), g, st); }
static void mixed_gemm(skf_plan* p, GemmArgs g, hipStream_t st) { kind_gemm(p, kind_mixed(p), g, st); }

// the same on the second stream: one K slice (the split-K scratch belongs to the main stream)
static void mixed_gemm_unsplit(skf_plan* p, GemmArgs g, hipStream_t st) { run_gemm(kind_mixed(p).ty, p->engine, g, 1, nullptr, 0, st); }

static hipEvent_t next_event(skf_plan* p) {
    if (p->ev_used == p->ev_pool.size()) {
        hipEvent_t e;
        SKF_HIP(hipEventCreate(&e));
        p->ev_pool.push_back(e);
    }
    return p->ev_pool[p->ev_used++];
}

// The right operand of a relation contraction (relation_gemm below) when it is NOT the factor of the type on the other side (skf_init.inc: the 0/1
// selection matrix of the column-mean initialisers): `n` columns -- the rank of whatever the caller forms, not of that type
// --, in the layout the relation's stored form reads: dense / bitmap relations of SKF_BF16 the bf16 Bt[n][ld] with the inner
// dimension zero padded as G^T is kept; every other form [inner][ld] in the master type (dense: what g.B / g.sb_k name
// already; SKF_REL_SPARSE_CSR: the gathered rows).  `part`: split-K slices / outputs of the list parts -- the caller's own,
// sized for ITS column count (the plan's scratch is sized for the iteration's).  The iteration passes none.
struct RelRight {
    const void* B;
    int64_t ld;
    int n;
    void* part;
    size_t part_bytes;
};
static int sparse_pass(skf_plan* p, const RelState& r, bool is_q, bool err, void* dst, hipStream_t st, int sq_first = 0,
                       const RelRight* rhs = nullptr);
static void ones_pass(skf_plan* p, const RelState& r, bool is_q, void* dst, int64_t ld_out, int64_t n_out, int w, hipStream_t st);
// one of the two contractions that stream a relation matrix: P = R G_j or Q = R^T G_i
static void relation_gemm(skf_plan* p, GemmArgs g, hipStream_t st, const RelState* r = nullptr, bool is_q = false,
                          const RelRight* rhs = nullptr) {
    if (rhs && (!r || g.N != rhs->n)) SKF_FAIL(SKF_E_STATE, "relation contraction: right operand without its relation / column count");
    if (r && r->sp0) {             // the stored entries as valued lists (every engine): no matrix to stream
        if (g.ldc != g.N) SKF_FAIL(SKF_E_STATE, "SKF_REL_SPARSE_CSR relation: strided contraction output");
        sparse_pass(p, *r, is_q, false, g.C, st, 0, rhs);
        return;
    }
    // (a 0/1 relation that SKF_BF16 keeps as lists of its ones beside its bitmap: the lists gather factor rows only -- a
    //  right operand of the caller's goes through the bitmap)
    const bool ones = p->bf16 && r && r->sparse && !rhs;
    void* const part = rhs ? rhs->part : p->part.ptr;
    const size_t part_bytes = rhs ? rhs->part_bytes : p->part_bytes;
    if (ones && r->sp_gather) {    // the ones as lists over the bf16 rows of the factor
        ones_pass(p, *r, is_q, g.C, g.ldc, g.M, g.N, st);
        return;
    }
    if (p->profiling) SKF_HIP(hipEventRecord(next_event(p), st));
    if (p->bf16) {
        const TypeState& ti = p->types[r->row];
        const TypeState& tj = p->types[r->col];
        // the bf16 right operand and its leading dimension: the stored transpose of the factor on the other side, or the caller's
        const uint16_t* btj = rhs ? (const uint16_t*)rhs->B : (const uint16_t*)tj.GTb.ptr;
        const uint16_t* bti = rhs ? (const uint16_t*)rhs->B : (const uint16_t*)ti.GTb.ptr + r->r0;
        const int64_t ldbj = rhs ? rhs->ld : tj.ldgt, ldbi = rhs ? rhs->ld : ti.ldgt;
        if (ones) {                    // a handful of ones per row / column: gather the factor's f32 rows (binary_spmm_kernel)
            const int wgrid = (int)(((int64_t)g.M + 3) / 4 < 4096 ? ((int64_t)g.M + 3) / 4 : 4096);
            hipLaunchKernelGGL(binary_spmm_kernel, dim3(wgrid), dim3(256), 0, st,
                               (const int64_t*)(is_q ? r->SpCp.ptr : r->SpRp.ptr), (const int*)(is_q ? r->SpRi.ptr : r->SpCi.ptr),
                               (const float*)g.B, (int64_t)g.N, (float*)g.C, (int64_t)g.ldc, (int64_t)g.M, g.N);
            check_launch("binary_spmm");
        } else if (r->binary) {        // the relation as a bitmap: 1/16 of the bytes, expanded to bf16 0 / 1 on the way into LDS
            if (!is_q)
                run_gemm_bf16((const uint16_t*)r->Bb.ptr, r->ldbb, btj, ldbj, (float*)g.C,
                              g.ldc, g.M, g.N, (int)r->ldrb, 0, part, part_bytes, true, st, false, true);
            else
                run_gemm_bf16((const uint16_t*)r->Bb.ptr, r->ldbb, bti, ldbi, (float*)g.C,
                              g.ldc, g.M, g.N, (int)r->kq, 0, part, part_bytes, true, st, true, true);
        } else if (!is_q)      // P = R G_j :  A = R (bf16), Bt = G_j^T (bf16)
            run_gemm_bf16((const uint16_t*)r->Rb.ptr, r->ldrb, btj, ldbj, (float*)g.C,
                          g.ldc, g.M, g.N, (int)r->ldrb, 0, part, part_bytes, true, st);
        else            // Q = R^T G_i :  A = the same row-major R read transposed out of LDS, Bt = G_i^T (bf16)
            run_gemm_bf16((const uint16_t*)r->Rb.ptr, r->ldrb, bti, ldbi, (float*)g.C,
                          g.ldc, g.M, g.N, (int)r->kq, 0, part, part_bytes, true, st, true);
    } else {
        const ProductKind k = kind_relation(p);
        run_gemm(k.ty, p->engine, g, 0, part, part_bytes, st, k.relation);
    }
    if (p->profiling) {
        SKF_HIP(hipEventRecord(next_event(p), st));
        // what the launch executes and the relation bytes it reads as stored (include/skfusion_hip.h, skf_plan_get_profile)
        const double cells = (double)g.M * (double)g.K;
        if (ones) {
            p->prof_flops += 2.0 * (double)r->sp_nnz * (double)g.N;
            p->prof_bytes += 4.0 * (double)r->sp_nnz;
        } else {
            p->prof_flops += 2.0 * cells * (double)g.N;
            p->prof_bytes += (p->bf16 && r && r->binary) ? cells / 8.0 : cells * (p->bf16 ? 2.0 : (double)p->esz);
        }
        p->prof_launches += 1;
    }
}

// SKF_BF16: refresh the bf16 transpose of a factor after it changed
static void refresh_gt(skf_plan* p, TypeState& t, hipStream_t st) {
    if (!p->bf16) return;
    launch_to_bf16<float>((uint16_t*)t.GTb.ptr, t.ldgt, (const float*)t.G.ptr, (int64_t)t.c, t.n, (int64_t)t.c, true, st);
    if (t.Grow.ptr)        // the bf16 rows for the list passes (their all-zero last row is never written)
        launch_to_bf16<float>((uint16_t*)t.Grow.ptr, t.ldrow, (const float*)t.G.ptr, (int64_t)t.c, t.n, (int64_t)t.c, false, st);
}

static void gram(skf_plan* p, TypeState& t, int nan, hipStream_t st, bool on_aux = false) {
    // Gram = G^T G : A = G^T (m-contiguous), B = G; f64 accumulation
    GemmArgs g = gemm_args(t.G.ptr, 1, t.c, t.G.ptr, t.c, 1, t.Gram.ptr, t.c, t.c, t.c, (int)t.n, EPI_STORE, nan);
    g.sym = p->sw.gram_sym;
    kind_gemm(p, kind_gram(p), g, st, on_aux);
}

// several Gram products (GemmArgs::sym set) in one grouped launch, where the switches allow it and run_gram_group_t takes them
static bool gram_group_try(skf_plan* p, const GemmArgs* gs, int n, void* part, size_t bytes, hipStream_t st) {
    if (!p->sw.gram_group || !p->sw.gram_sym || n < 2 || n > 4) return false;
    return p->mt == SKF_F64 ? run_gram_group_t<double>(p->engine, gs, n, part, bytes, st)
                            : run_gram_group_t<float>(p->engine, gs, n, part, bytes, st);
}
// the Gram matrices of ALL types at the head of an iteration: one grouped launch where that is taken, else one by one
static void gram_all(skf_plan* p, int nan, hipStream_t st, bool on_aux) {
    const size_t nt = p->types.size();
    if (nt >= 2 && nt <= 4) {
        GemmArgs gs[4];
        for (size_t i = 0; i < nt; ++i) {
            TypeState& t = p->types[i];
            gs[i] = gemm_args(t.G.ptr, 1, t.c, t.G.ptr, t.c, 1, t.Gram.ptr, t.c, t.c, t.c, (int)t.n, EPI_STORE, nan);
            gs[i].sym = 1;
        }
        if (gram_group_try(p, gs, (int)nt, on_aux ? p->part_aux.ptr : p->part.ptr, on_aux ? p->part_aux_bytes : p->part_bytes, st))
            return;
    }
    for (size_t i = 0; i < nt; ++i) gram(p, p->types[i], nan, st, on_aux);
}

// G <- G * sqrt(E / max(D, eps)) on the rows [r0, r0 + n) of the type, master copies only
static void mult_update_rows(skf_plan* p, TypeState& t, int64_t r0, int64_t n, hipStream_t st) {
    const int64_t total = n * t.c;
    const size_t off = (size_t)r0 * t.c;
    if (p->f64)
        hipLaunchKernelGGL((mult_update_kernel<double>), dim3(elem_grid(total)), dim3(256), 0, st, (double*)t.G.ptr + off,
                           (const double*)t.E.ptr + off, (const double*)t.D.ptr + off, n, t.c, (int64_t)t.c, (int64_t)t.c);
    else
        hipLaunchKernelGGL((mult_update_kernel<float>), dim3(elem_grid(total)), dim3(256), 0, st, (float*)t.G.ptr + off,
                           (const float*)t.E.ptr + off, (const float*)t.D.ptr + off, n, t.c, (int64_t)t.c, (int64_t)t.c);
    check_launch("mult_update");
}
static void mult_update(skf_plan* p, TypeState& t, hipStream_t st) { mult_update_rows(p, t, 0, t.n, st); }

// the hub rows of a sparse constraint inside [r0, r0 + nr): their segments as partial sums, then the sums into E / D.  The
// table is sorted by row, so the rows of the range are one sub-range of it (found here, on the host).  `E` / `D`: row 0 of
// the table's row numbering (the whole accumulators; a constraint of local rows: their owned range, r0 = 0, the whole table).
template <typename T>
static void theta_hub_rows_t(ThetaState& th, TypeState& t, int64_t r0, int64_t nr, T* E, T* D, hipStream_t st) {
    const size_t h0 = std::lower_bound(th.hub_rows.begin(), th.hub_rows.end(), r0) - th.hub_rows.begin();
    const size_t h1 = std::lower_bound(th.hub_rows.begin(), th.hub_rows.end(), r0 + nr) - th.hub_rows.begin();
    if (h1 <= h0) return;
    const int64_t s0 = th.hub_first[h0], s1 = th.hub_first[h1];       // (hub_first has one entry more than hub_rows: n_seg)
    const int64_t groups = (t.c + 63) / 64;
    hipLaunchKernelGGL((theta_hub_partial_kernel<T>), dim3(wave_grid((s1 - s0) * groups)), dim3(256), 0, st,
                       (const ThetaSeg*)th.HubSeg.ptr + s0, s1 - s0, (const int*)th.Ci.ptr, (const T*)th.Vv.ptr, (const T*)t.G.ptr,
                       (T*)th.HubE.ptr + s0 * t.c, (T*)th.HubD.ptr + s0 * t.c, t.c);
    check_launch("theta_hub_partial");
    // (ThetaHub::first counts from the head of the table, so the partials are addressed from there too; E / D by the table's row)
    hipLaunchKernelGGL((theta_hub_combine_kernel<T>), dim3(elem_grid((int64_t)(h1 - h0) * t.c)), dim3(256), 0, st,
                       (const ThetaHub*)th.HubRows.ptr + h0, (int64_t)(h1 - h0), (const T*)th.HubE.ptr, (const T*)th.HubD.ptr,
                       E, D, t.c);
    check_launch("theta_hub_combine");
}

// D_i += Theta+ G_i ; E_i += Theta- G_i   (_dfmf.py:284-292) on the rows [r0, r0 + nr) of the constrained type (all of
// them, or -- ownership-aligned row blocks -- the rows this plan owns: a row of the product needs the row of Theta and the
// whole factor).  `only_type` >= 0: the constraints of that type only.
static void theta_terms_rows(skf_plan* p, int only_type, bool own_rows, hipStream_t st) {
    for (ThetaState& th : p->thetas) {
        if (only_type >= 0 && th.type != only_type) continue;
        TypeState& t = p->types[th.type];
        const int64_t r0 = own_rows ? t.t0 : 0, nr = own_rows ? t.tn : t.n;
        if (nr <= 0) continue;
        if (th.local && !(own_rows && r0 == th.l0 && nr == th.ln))
            SKF_FAIL(SKF_E_STATE, "constraint on type %d holds the owned rows only: it runs in the owned schedule (skf_iterate_dist)", th.type);
        // (the global form shifts its row pointers to the range and finds its hub rows inside it; the local form starts at 0)
        const int64_t q0 = th.local ? 0 : r0;
        void* Er = (char*)t.E.ptr + (size_t)r0 * t.c * p->esz;
        void* Dr = (char*)t.D.ptr + (size_t)r0 * t.c * p->esz;
        // an all-zero half is skipped
        if (th.sparse) {    // both halves in one pass over the CSR form, master precision
            if (th.nnz == 0) continue;
            const int grid = wave_grid(nr);
            const int64_t hub = th.n_seg > 0 ? th.hub_row : 0;      // (a plan without hub rows launches what it always did)
            if (p->f64)
                hipLaunchKernelGGL((theta_spmm_kernel<double>), dim3(grid), dim3(256), 0, st, (const int64_t*)th.Rp.ptr + q0,
                                   (const int*)th.Ci.ptr, (const double*)th.Vv.ptr, (const double*)t.G.ptr, (double*)Er,
                                   (double*)Dr, nr, t.c, hub);
            else
                hipLaunchKernelGGL((theta_spmm_kernel<float>), dim3(grid), dim3(256), 0, st, (const int64_t*)th.Rp.ptr + q0,
                                   (const int*)th.Ci.ptr, (const float*)th.Vv.ptr, (const float*)t.G.ptr, (float*)Er,
                                   (float*)Dr, nr, t.c, hub);
            check_launch("theta_spmm");
            if (hub > 0) {
                char* E0 = th.local ? (char*)Er : (char*)t.E.ptr;
                char* D0 = th.local ? (char*)Dr : (char*)t.D.ptr;
                if (p->f64) theta_hub_rows_t<double>(th, t, q0, nr, (double*)E0, (double*)D0, st);
                else theta_hub_rows_t<float>(th, t, q0, nr, (float*)E0, (float*)D0, st);
            }
            continue;
        }
        if (p->bf16) {      // bf16 copies of the halves against the stored G^T, f32 accumulate, then added
            for (int half = 0; half < 2; ++half) {
                if (!(half == 0 ? th.has_pos : th.has_neg)) continue;
                run_gemm_bf16((const uint16_t*)(half == 0 ? th.Pb.ptr : th.Nb.ptr) + r0 * th.ldb, th.ldb, (const uint16_t*)t.GTb.ptr,
                              t.ldgt, (float*)p->theta_tmp.ptr, t.c, (int)nr, t.c, (int)th.ldb, 0, p->part.ptr,
                              p->part_bytes, false, st);
                hipLaunchKernelGGL(add_into_kernel, dim3(elem_grid(nr * t.c)), dim3(256), 0, st,
                                   (float*)(half == 0 ? Dr : Er), (const float*)p->theta_tmp.ptr, (int64_t)nr * t.c);
                check_launch("add_into");
            }
            continue;
        }
        GemmArgs g = gemm_args((const char*)th.data + (size_t)r0 * th.ld * p->esz, th.ld, 1, t.G.ptr, t.c, 1, Dr, t.c, (int)nr, t.c,
                               (int)t.n, EPI_ACC, 0);
        g.aop = AOP_POS;
        if (th.has_pos) plan_gemm(p, g, st);
        g.C = Er;
        g.aop = AOP_NEG;
        if (th.has_neg) plan_gemm(p, g, st);
    }
}

static void theta_terms(skf_plan* p, hipStream_t st) { theta_terms_rows(p, -1, false, st); }

// [Xp, Xn] (+)= split( L * Gram * Rr )  helper for B = S Gram_j S^T and D = S^T Gram_i S
// tmp = first product, then split-store/acc of the second.
static void relation_small_terms(skf_plan* p, RelState& r, int nan_upd, int epi_split, void* Bp, void* Bn,
                                 void* Dp, void* Dn, bool want_row, bool want_col, hipStream_t st, void* U2 = nullptr) {
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    const int ci = ti.c, cj = tj.c;
    if (want_row && want_col && U2 && U2 != r.U.ptr) {
        // both sides, and a second ci x cj buffer: the two Gram products side by side in one launch, then the two products
        // that add into the B sums (one launch as well unless both add into the SAME sums: a relation of a type with itself)
        const bool pairs = !p->sw.no_pairs;
        GemmArgs gu = gemm_args(r.S.ptr, cj, 1, tj.Gram.ptr, cj, 1, r.U.ptr, cj, ci, cj, cj, EPI_STORE, 0);      // U = S Gram_j
        GemmArgs gv = gemm_args(ti.Gram.ptr, ci, 1, r.S.ptr, cj, 1, U2, cj, ci, cj, ci, EPI_STORE, 0);          // U2 = Gram_i S
        run_gemm_pair_f64(p->engine, gu, gv, st, pairs);
        GemmArgs gb = gemm_args(r.U.ptr, cj, 1, r.S.ptr, 1, cj, Bp, ci, ci, ci, cj, epi_split, nan_upd);         // B = U S^T
        gb.C2 = Bn;
        GemmArgs gd = gemm_args(r.S.ptr, 1, cj, U2, cj, 1, Dp, cj, cj, cj, ci, epi_split, nan_upd);              // D = S^T U2
        gd.C2 = Dn;
        run_gemm_pair_f64(p->engine, gb, gd, st, pairs && Bp != Dp && Bn != Dn);
        return;
    }
    if (want_row) {
        // U = S Gram_j (ci x cj);  B = U S^T (ci x ci)          tmp2 of _dfmf.py:260
        GemmArgs g = gemm_args(r.S.ptr, cj, 1, tj.Gram.ptr, cj, 1, r.U.ptr, cj, ci, cj, cj, EPI_STORE, 0);
        small_gemm(p, g, st);
        g = gemm_args(r.U.ptr, cj, 1, r.S.ptr, 1, cj, Bp, ci, ci, ci, cj, epi_split, nan_upd);
        g.C2 = Bn;
        small_gemm(p, g, st);
    }
    if (want_col) {
        // U = Gram_i S (ci x cj);  D = S^T U (cj x cj)          tmp5 of _dfmf.py:272
        GemmArgs g = gemm_args(ti.Gram.ptr, ci, 1, r.S.ptr, cj, 1, r.U.ptr, cj, ci, cj, ci, EPI_STORE, 0);
        small_gemm(p, g, st);
        g = gemm_args(r.S.ptr, 1, cj, r.U.ptr, cj, 1, Dp, cj, cj, cj, ci, epi_split, nan_upd);
        g.C2 = Dn;
        small_gemm(p, g, st);
    }
}

// f32 engines: the f32 roundings of a type's two B sums in ONE launch (they were two)
static void cast_b_sums(TypeState& t, hipStream_t st) {
    const int cc = t.c * t.c;
    CastBatch cb;
    memset(&cb, 0, sizeof cb);
    cb.src[0] = (const double*)t.Bn_tot.ptr; cb.dst[0] = (float*)t.Bn32.ptr; cb.count[0] = cc;
    cb.src[1] = (const double*)t.Bp_tot.ptr; cb.dst[1] = (float*)t.Bp32.ptr; cb.count[1] = cc;
    hipLaunchKernelGGL(cast_batched_kernel, dim3(elem_grid(cc), 2), dim3(256), 0, st, cb);
    check_launch("cast_batched");
}

// Fused E/D update of one relation side (MFMA engine): E (+)= (X Sop)+ + G Bn, D (+)= (X Sop)- + G Bp
// on the rows [G, E, D point at the first one; n of them] of type t.  Sop / Bn / Bp are c x c matrices
// in the master type (the f32 engines pass f32 roundings of the f64 originals -- the same values
// the f32 matrix cores would see -- so that the staged operands take half the registers).
static void side_update(skf_plan* p, const void* X, int64_t ldx, int k1, const void* Sop, int64_t ss_k, int64_t ss_n,
                        TypeState& t, const void* G, void* E, void* D, int n, const void* Bn, const void* Bp,
                        bool phase2, bool accumulate, int nan, hipStream_t st) {
    SideArgs a;
    a.X = X; a.Sop = Sop; a.G = G; a.Bn = Bn; a.Bp = Bp; a.E = E; a.D = D;
    a.ldx = ldx; a.ss_k = ss_k; a.ss_n = ss_n; a.ldg = t.c; a.ldb = t.c; a.lde = t.c;
    a.n = n; a.c = t.c; a.k1 = k1;
    a.accumulate = accumulate ? 1 : 0;
    a.nan_to_num = nan;
    a.phase2 = phase2 ? 1 : 0;
    bool big = (n > 64 && t.c > 64);
    dim3 block(GEMM_THREADS);
    if (p->f64) {
        if (big) {
            dim3 grid(cdiv(t.c, 64), cdiv(n, 64));
            hipLaunchKernelGGL((side_update_kernel<double, double, 2, 2, 16>), grid, block, 0, st, a);
        } else {
            dim3 grid(cdiv(t.c, 32), cdiv(n, 32));
            hipLaunchKernelGGL((side_update_kernel<double, double, 1, 1, 16>), grid, block, 0, st, a);
        }
    } else {
        const int force = p->sw.side_tile;                   // 64 / 128 force a tile shape (A/B runs, tests)
        // the two operand layouts of the iteration with everything 16-byte aligned get kernels whose
        // staging modes are compile-time constants (SKF_SIDE_FM); anything else the generic one
        auto al = [](const void* q) { return q == nullptr || (((uintptr_t)q) & 15) == 0; };
        const bool vec = al(X) && al(Sop) && al(G) && al(Bn) && al(Bp) && t.c % 4 == 0 && k1 % 4 == 0 &&
                         ldx % 4 == 0 && (k1 == 0 || (ss_k == 1 ? ss_n % 4 == 0 : (ss_n == 1 && ss_k % 4 == 0)));
        const bool k_major = (k1 == 0 || ss_k == 1);
        // measured at config 3 (rocprof, all six launches): the 64 x 64 fixed-mode kernels (78 VGPRs, 6
        // workgroups per CU) beat the 128 x 128 ones (182 VGPRs, 2 per CU): 0.98 vs 1.30 ms per iteration
        // (the 128 x 128 tile only with compile-time staging modes: its run-time form spilled registers)
        if (big && !(force == 128 && vec)) big = false;
        constexpr int FM_K = SKF_SIDE_FM(STAGE_VEC_K, STAGE_VEC_K, STAGE_VEC_K, STAGE_VEC_R);
        constexpr int FM_R = SKF_SIDE_FM(STAGE_VEC_K, STAGE_VEC_R, STAGE_VEC_K, STAGE_VEC_R);
        if (big) {
            dim3 grid(cdiv(t.c, 128), cdiv(n, 128));
            if (k_major)
                hipLaunchKernelGGL((side_update_kernel<float, float, 2, 2, 16, FM_K>), grid, block, 0, st, a);
            else
                hipLaunchKernelGGL((side_update_kernel<float, float, 2, 2, 16, FM_R>), grid, block, 0, st, a);
        } else {
            dim3 grid(cdiv(t.c, 64), cdiv(n, 64));
            // (K tiles of 32 / 64 instead of 16, round 4: config 3 91.1 / 89.2 against 90.8 it/s, config 5 144.9 / 143.0
            //  against 144.3 -- within the noise / worse)
            if (vec && k_major && n > 64 && t.c >= 64)
                hipLaunchKernelGGL((side_update_kernel<float, float, 1, 1, 16, FM_K>), grid, block, 0, st, a);
            else if (vec && n > 64 && t.c >= 64)
                hipLaunchKernelGGL((side_update_kernel<float, float, 1, 1, 16, FM_R>), grid, block, 0, st, a);
            else
                hipLaunchKernelGGL((side_update_kernel<float, float, 1, 1, 16>), grid, block, 0, st, a);
        }
    }
    check_launch("side_update");
}

// A view of the rows [r0, r0 + nr) of a factor-shaped matrix (G, E, D) of type t
static inline void* rows_of(const skf_plan* p, const Slot& s, const TypeState& t, int64_t r0) {
    return (char*)s.ptr + (size_t)r0 * t.c * p->esz;
}

static void contraction_P(skf_plan* p, RelState& r, hipStream_t st) {      // P = R_blk G_j
    TypeState& tj = p->types[r.col];
    GemmArgs g = gemm_args(r.R, r.ldr, 1, tj.G.ptr, tj.c, 1, r.P.ptr, tj.c, (int)r.nr, tj.c, (int)tj.n, EPI_STORE, 0);
    relation_gemm(p, g, st, &r, false);
}

static void contraction_Q(skf_plan* p, RelState& r, hipStream_t st) {      // Q = R_blk^T G_i[blk]
    TypeState& ti = p->types[r.row];
    TypeState& tj = p->types[r.col];
    if (r.absent) {
        SKF_HIP(hipMemsetAsync(r.Q.ptr, 0, r.Q.bytes, st));
        return;
    }
    GemmArgs g = gemm_args(r.R, 1, r.ldr, rows_of(p, ti.G, ti, r.r0), ti.c, 1, r.Q.ptr, ti.c, (int)tj.n, ti.c,
                           (int)r.nr, EPI_STORE, 0);
    relation_gemm(p, g, st, &r, true);
}
