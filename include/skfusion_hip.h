/* skfusion_hip.h -- C ABI of libskfusion_hip.so: the MI355X (gfx950) engine for the DFMF / DFMC /
 * fold-in update loop of scikit-fusion.
 *
 * The reference has no FFI: its seam is the functional solver API that the one-line wrappers
 * call (reference skfusion/fusion/decomposition/dfmf.py:14-15 -> _dfmf.py:127 `dfmf`,
 * dfmc.py:14-15 -> _dfmc.py:181 `dfmc`, dfmf.py:109-115 -> _dfmf.py:330 `transform`).  The entry
 * points below are what a ctypes binding at that seam binds (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success, <0 on error
 *     (SKF_E_*), and the message is available from skf_last_error() (thread-local).
 *   - every data pointer is a DEVICE pointer owned by the caller; the library never allocates
 *     or frees device memory: the caller provides one workspace of skf_plan_workspace_bytes().
 *   - matrices are row-major with a leading dimension counted in elements.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  No call synchronises
 *     the host unless stated.
 *   - a plan is not re-entrant; different plans may be driven from different threads.
 */
#ifndef SKFUSION_HIP_H
#define SKFUSION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* arithmetic type of the engine: storage of the relation / constraint matrices and of every
 * factor; the reference computes in f64 throughout (numpy float64, _init.py:16). */
enum { SKF_F64 = 0, SKF_F32 = 1, SKF_BF16 = 2 /* bf16 relation storage + f32 masters */ };

/* which reference solver the plan replaces */
enum {
    SKF_DFMF = 0,      /* _dfmf.py:127-327  */
    SKF_DFMC = 1,      /* _dfmc.py:181-397  */
    SKF_TRANSFORM = 2  /* _dfmf.py:330-458  */
};

enum { SKF_ENGINE_MFMA = 0, SKF_ENGINE_VALU = 1 };

enum {
    SKF_OK = 0,
    SKF_E_INVALID = -1,    /* bad argument / shape / index */
    SKF_E_STATE = -2,      /* call order (workspace not bound, factors not set ...) */
    SKF_E_WORKSPACE = -3,  /* workspace too small / misaligned */
    SKF_E_HIP = -4         /* a HIP runtime call or kernel launch failed */
};

typedef struct skf_plan skf_plan;

typedef struct {
    int64_t n_obj; /* objects of this type   (count_objects, _dfmf.py:95-124) */
    int32_t rank;  /* factorisation rank c_i (int(ot.rank), dfmf.py:67)       */
} skf_type_desc;

typedef struct {
    int32_t row_type, col_type; /* indices into the type array; row_type != col_type */
    const void* data;           /* n_row x n_col, engine dtype (R[(i,j)][l], dfmf.py:82-85);
                                   SKF_BF16: bf16 (uint16) data, copied ONCE into a zero-padded
                                   row-major layout at bind time (both contractions read that
                                   one copy) and not referenced afterwards */
    int64_t ld;
    const uint8_t* mask;        /* DFMC only (M[(i,j)][l], dfmc.py:77-90); NULL = no mask.
                                   Default: n_row x n_col BYTES, !=0 = unknown entry, mask_ld in
                                   bytes = entries.  SKF_REL_MASK_BITS: packed, one BIT per entry
                                   (bit (c & 7) of byte mask[r * mask_ld + (c >> 3)], 1 = unknown),
                                   mask_ld = bytes per row >= ceil(n_col / 8).  Either form is
                                   converted to the engine's packed layout at bind time and not
                                   referenced afterwards: an iteration reads 1 bit per entry */
    int64_t mask_ld;
    /* Row-block sharding of ONE relation over several processes: this process holds
     * rows [row_begin, row_begin + n_rows) of the relation; `data` / `mask` point at its first LOCAL
     * row.  n_rows == 0 (zero-initialised descriptor): the whole relation is here.  A plan that
     * lists a relation it holds no rows of sets SKF_REL_ABSENT (data may be NULL).  See skf_stage. */
    int64_t row_begin;
    int64_t n_rows;
    int32_t flags;              /* SKF_REL_* */
    int64_t known_bound;        /* masked relations (DFMC): 0 = unknown, or an upper bound on the number of KNOWN entries
                                   (mask == 0).  When that is a small share of the relation, the plan keeps ONLY the known
                                   entries (CSR + CSC with values) and never materialises the completed relation of
                                   _dfmc.py:319-325: with E = (R - G_i S G_j^T) on the known entries, R_c = G_i S G_j^T + E,
                                   so P, Q and the next backbone's G_i^T R_c G_j split into c x c algebra plus products
                                   of the sparse E (cost ~ known * c + n * c^2 instead of n_i * n_j * c; same results up
                                   to associativity).  A bound that turns out too small is an error at bind time.
                                   Ignored for unmasked relations, row blocks and SKF_DFMF / SKF_TRANSFORM plans. */
} skf_relation_desc;

enum {
    SKF_REL_ABSENT = 1,       /* no local rows of this relation (its backbone / Q are still kept) */
    SKF_REL_NO_COL_SIDE = 2,  /* another process adds the column-side terms E_j, D_j of this relation */
    SKF_REL_MASKED = 4,       /* SKF_REL_ABSENT descriptors: the relation is masked where it lives */
    SKF_REL_MASK_BITS = 8,    /* `mask` is packed, one bit per entry (see skf_relation_desc.mask) */
    SKF_REL_KNOWN_LISTS = 32, /* SKF_OPT_OWNED_ROWS plans: this masked relation is kept as lists of its known entries (see
                                 known_bound) on EVERY process -- the caller decides it for all of them alike from the share of
                                 known entries of the WHOLE relation (the partial sums the processes exchange follow one
                                 convention per relation); also set on SKF_REL_ABSENT descriptors of such a relation.  known_bound
                                 then bounds the known entries of the LOCAL rows.  Other plans: ignored (the library decides). */
    SKF_REL_BINARY = 16,      /* every entry is 0 or 1 (checked at bind time; "movie has genre", "user tagged").
                                 SKF_BF16 keeps such a relation as a BITMAP -- 1 bit instead of a bf16 per entry
                                 in HBM and on the way to the matrix cores, where it is expanded to bf16 0 / 1 in
                                 LDS: the same products as the dense form, bit for bit.  A sparse one also keeps
                                 the positions of its ones as CSR + CSC and both contractions run over those
                                 lists: with both ranks 64 / 128 / 256 and at most 1 entry in 80 set, as f32 sums
                                 of the bf16 rows of the factors (what the bitmap kernels compute, in another
                                 order); with other ranks and at most 1 entry in 256 set, as gathers of the f32
                                 factor rows (exact f32 sums).  Ignored for masked relations and by the f32 / f64
                                 engines. */
    SKF_REL_KNOWN_CSR = 64,   /* SKF_DFMC: the relation is given as its KNOWN entries only, as CSR (the stored entries are the
                                 known ones, every other entry is unknown) -- no dense form exists: `data` and `mask` are NULL,
                                 known_bound is the EXACT number of entries (0 allowed) and skf_plan_set_known_entries hands the
                                 lists over before skf_plan_bind_workspace.  Always kept as lists of its known entries (neither
                                 SKF_DFMC_SPARSE nor the share rule applies: there is no dense form to fall back on); the lists
                                 built at bind time are the ones the mask form of the same data builds, byte for byte.
                                 SKF_OPT_OWNED_ROWS plans take the relation as the CSR of the OWNED rows of its row type, over
                                 all columns: row_begin / n_rows are exactly the range skf_owned_rows names (the rule of dense
                                 blocks), skf_plan_set_known_entries receives indptr[n_rows + 1] rebased to 0 and known_bound is
                                 the slice's entry count; a process that owns no row of the row type passes SKF_REL_KNOWN_CSR |
                                 SKF_REL_ABSENT and hands over no lists.  After bind such a relation is a masked row block
                                 flagged SKF_REL_KNOWN_LISTS (the absent process adds the dense part of Q on its rows of the
                                 column type).
                                 SKF_E_INVALID: SKF_DFMF / SKF_TRANSFORM plans, row blocks / sliced plans without
                                 SKF_OPT_OWNED_ROWS, a block of an owned plan that is not the owned range, a row type's rank
                                 above 1024, more than 2e9 entries. */
    SKF_REL_SPARSE_CSR = 128, /* SKF_DFMF plans, and unmasked relations of SKF_DFMC plans: the relation is given as the CSR of its
                                 STORED entries and every other entry is ZERO (what a scipy.sparse matrix means; the reference
                                 multiplies its dense expansion, _dfmf.py:249-276, and forms its error from the dense
                                 reconstruction, _dfmf.py:306-316).  `data` and `mask` are NULL, known_bound is the EXACT number of
                                 stored entries (0 allowed: an all-zero relation) and skf_plan_set_known_entries hands the lists
                                 over before skf_plan_bind_workspace -- values in the MASTER type: f64 / f32, SKF_BF16 plans f32
                                 (the stored values are never rounded to bf16).  The relation is never expanded: P = R G_j is one
                                 pass over its row lists, Q = R^T G_i one over its column lists (built at bind time, values
                                 included), skf_relation_sqerr = tr(S^T Gram_i S Gram_j) + sum over the stored entries of
                                 (r - x)^2 - x^2.  Workspace grows with the number of entries and n * c, never with n_i * n_j.
                                 Such a plan runs the relation pipeline or the staged schedule, never the small-graph one.
                                 Stored zeros stay entries.  SKF_OPT_OWNED_ROWS plans take the CSR of the OWNED rows of the row
                                 type, over all columns, under the slice convention of SKF_REL_KNOWN_CSR (row_begin / n_rows =
                                 the owned range, indptr[n_rows + 1] rebased to 0, known_bound = the slice's entry count,
                                 SKF_REL_SPARSE_CSR | SKF_REL_ABSENT and no lists where the process owns no row of the row type:
                                 it still contributes a zero partial Q and receives its scattered rows); the owned schedule runs
                                 as for a dense block -- P on the local rows, the share of W, the partial Q over all columns --
                                 and skf_relation_sqerr covers the local rows (the trace term from the Gram of the local rows of
                                 G_i: the processes' values sum to the relation's).  Nothing of size n_rows x n_j exists.
                                 SKF_E_INVALID: SKF_TRANSFORM plans, row blocks / sliced plans without SKF_OPT_OWNED_ROWS, a
                                 block of an owned plan that is not the owned range, a rank above 1024, more than 2e9 entries,
                                 a mask, together with SKF_REL_KNOWN_CSR. */
    SKF_REL_FILL_RANK1 = 512, /* only together with SKF_REL_SPARSE_CSR, on SKF_DFMF / SKF_DFMC plans of whole relations: a relation
                                 with MISSING values whose unknown cells were imputed before the fit (the reference's
                                 Relation.filled(), fusion_graph.py:464-510).  Every fill strategy writes a rank-one pattern
                                 into the unknown cells, so the filled matrix is F = a b^T + D with D sparse on the stored pattern,
                                 d = v - a_r b_c: a constant f: a = f 1, b = 1; 'mean': a = m 1, b = 1; 'row_mean': a = the row
                                 means, b = 1; 'col_mean': a = 1, b = the column means.  The caller hands over the TRUE stored
                                 values v (skf_plan_set_known_entries) and the two vectors (skf_plan_set_relation_fill); bind forms
                                 d = (double)v - (double)a_r (double)b_c, rounded once to the master type, before the column
                                 lists are built, and skf_get_relation_lists returns d.  Then
                                     P = F G_j   = D G_j   + a (b^T G_j)
                                     Q = F^T G_i = D^T G_i + b (a^T G_i)
                                 -- the list passes of SKF_REL_SPARSE_CSR on d, plus the weighted column sums t = G_j^T b and
                                 s = G_i^T a (f64, from the rows the list pass gathers: the bf16 rows in the SKF_BF16 engine, so
                                 that P = sum over the stored of v g^ + a sum over the unstored of b g^ over ONE set of rounded
                                 rows, as the dense bf16 contraction gives; two stages, a fixed slab of 128 rows per workgroup,
                                 partials added first to last, no atomics: the same bits on every run and device), added as
                                 P[r] += a_r t, Q[c] += b_c s in the launch that sums the parts of the lists -- and
                                     |F - G_i S G_j^T|^2 = tr(S^T Gram_i S Gram_j) + |a|^2 |b|^2 - 2 (a^T G_i) S (G_j^T b)
                                                           + sum over the stored of (d - x)^2 - x^2 + 2 sum over the stored of d a_r b_c
                                 (skf_relation_sqerr; the sums over the objects from the masters in every engine, the c_i x c_j
                                 product in f64, the three constants |a|^2, |b|^2, 2 sum d a b in f64, summed in ascending order
                                 at bind).  Workspace grows by (n_i + n_j) (element size + 8) + (ceil(n_i / 128) c_i +
                                 ceil(n_j / 128) c_j + c_i + c_j) 8 bytes, never with n_i * n_j.  A relation without the flag
                                 issues exactly the launches it issued before the flag existed.
                                 SKF_E_INVALID at skf_plan_create: without SKF_REL_SPARSE_CSR, SKF_OPT_OWNED_ROWS plans,
                                 SKF_TRANSFORM plans; at bind: no skf_plan_set_relation_fill, a fill value that is not finite
                                 (checked with the lists, before anything gathers). */
    SKF_REL_FOLD_CSR = 256,   /* SKF_TRANSFORM plans only: the NEW relation is given as its STORED entries, every other entry ZERO,
                                 compressed along the TARGET's side -- indptr[n_target + 1] (int64), indices (int32, into the
                                 partner type, strictly ascending within a target object) and values in the MASTER type (f64 /
                                 f32; SKF_BF16 plans: f32, never rounded to bf16).  A relation whose row type is the target: its
                                 canonical CSR; one whose column type is the target: its canonical CSC (the CSR of the
                                 transpose).  `data` and `mask` are NULL, known_bound is the EXACT number of entries (0 allowed)
                                 and skf_plan_set_known_entries hands the lists over before skf_plan_bind_workspace, which
                                 validates them (rows = target objects, columns = partner objects) and copies them into the
                                 workspace: re-preparation after skf_set_backbone / skf_set_factor finds them there.  Nothing
                                 else is built -- no parts, no second orientation: everything that reads the relation is
                                 independent of the moving factor, so the preparation is T = G_p S^T (row side; G_p S on the
                                 column side; n_partner x c_target, master type) and ONE pass Ec += (R T)+, Dc += (R T)-
                                 (skf_fold_lists; reference _dfmf.py:394-398,408-412 on the dense relation), and an iteration
                                 never touches the relation.  Dense relations of the same plan are untouched.  skf_relation_sqerr:
                                 the trace term as for SKF_REL_SPARSE_CSR plus one pass over the lists with x = <H[o], G_p[idx]>,
                                 H = G_t S (row side) / G_t S^T (column side), master rows in every engine.  No P / Q is ever
                                 formed (skf_get_contraction: SKF_E_INVALID); workspace grows with entries + n * c, never with
                                 n_t * n_p.  SKF_E_INVALID: SKF_DFMF / SKF_DFMC plans, together with SKF_REL_KNOWN_CSR /
                                 SKF_REL_SPARSE_CSR, a mask, a row block, a rank above 1024, more than 2e9 entries, a missing
                                 hand-over, a broken list.  (SKF_REL_SPARSE_CSR stays an error on SKF_TRANSFORM plans.) */
    SKF_REL_FOLD_KNOWN = 1024 /* with SKF_REL_FOLD_CSR only (SKF_TRANSFORM plans): stored = KNOWN.  Every entry that is not stored
                                 is UNKNOWN and takes the current model's prediction in every iteration -- the completion step
                                 of reference _dfmc.py:319-325 followed by the target's update of _dfmf.py:385-428, with every
                                 other factor and every backbone frozen -- without the completed relation: with T = G_p S^T (row
                                 side; G_p S on the column side), B_r = T^T T and the known entries (i_k, v_k) of target object o
                                     tmp1[o] = G[o] B_r + sum_k (v_k - <G[o], T[i_k]>) T[i_k]      (= R_completed[o] T)
                                     E[o] += max(tmp1, 0) + G[o] max(-B_r, 0) ,  D[o] += max(-tmp1, 0) + G[o] max(B_r, 0)
                                 Hand-over, validation, workspace copy and limits are those of SKF_REL_FOLD_CSR.  The
                                 preparation forms T and B_r (unsplit, c_t x c_t f64; its split joins the B sums of the target
                                 as for every relation) and adds nothing to the constant sums; every iteration forms X = G B_r
                                 into ONE n_t x c_t scratch of the plan (master type, counted by skf_plan_workspace_bytes) and
                                 makes one pass over the lists (skf_fold_known_pass; SKF_BF16 plans: on the f32 masters, T in
                                 f32), so a plan with such a relation never takes the one-launch iteration and does not batch
                                 (skf_plan_batchable: 0; skf_iterate_batch: SKF_E_INVALID).  skf_relation_sqerr: the KNOWN-ENTRY
                                 objective, see there.  SKF_E_INVALID at skf_plan_create: without SKF_REL_FOLD_CSR, on SKF_DFMF /
                                 SKF_DFMC plans; every refusal of SKF_REL_FOLD_CSR holds (skf_get_contraction and the device
                                 initialisers among them). */
};

typedef struct {
    int32_t type;     /* constrained object type (Theta[(i,i)][t], dfmf.py:82-85) */
    const void* data; /* n_i x n_i, engine dtype (SKF_BF16: f32), dense row-major.  NULL: the constraint is given as the CSR of
                         its STORED entries and every other entry is ZERO (what a scipy.sparse matrix means; the reference
                         multiplies its dense expansion, _dfmf.py:284-292): `nnz` is then the EXACT number of entries (0
                         allowed: an all-zero constraint), `ld` is ignored and skf_plan_set_constraint_entries hands the lists
                         over before skf_plan_bind_workspace.  No dense form exists in any type: the constraint is kept as
                         lists whatever its density, the same lists the dense form of the same matrix is compacted to, and
                         the workspace grows by nnz * (4 + element size) + (n_i + 1) * 8 + n_i * 4 bytes, never with
                         n_i * n_i.  SKF_DFMF / SKF_DFMC plans and the target type of SKF_TRANSFORM plans, every engine.  For
                         the small-graph schedule it counts as sparse under the condition of skf_small_graph_limits
                         (0 < nnz <= n_i * n_i / 16); otherwise the plan takes the general schedule.  SKF_E_INVALID at
                         skf_plan_create: plans with row blocks, sliced and SKF_OPT_OWNED_ROWS plans, more than 2e9 entries.
                         SKF_OPT_OWNED_ROWS plans with SKF_OPT_THETA_OWNED_ROWS take such a constraint as the CSR of the
                         OWNED rows of its type (skf_owned_rows), over all columns: `nnz` is the exact entry count of that
                         slice (it differs between the processes; 0 allowed, also where no row is owned) and the workspace
                         grows by nnz * (4 + element size) + (count + 1) * 8 bytes -- with the slice, never with n_i * n_i
                         or with the whole constraint. */
    int64_t ld;
    int64_t nnz;      /* 0: multiply it as a dense matrix, as the reference does (_dfmf.py:284-292).  > 0: an upper
                         bound on its non-zero entries -- the engine then keeps the constraint as CSR (built on the
                         device at bind time, `data` is not referenced afterwards) and D_i += Theta+ G_i,
                         E_i += Theta- G_i become ONE sparse pass in the master precision.  Accepted up to
                         n_i * n_i / 16; a bound that turns out too small is an error at bind time.  Either form: a row of
                         the CSR longer than 4096 entries (SKF_THETA_HUB_ROW=n in the environment of skf_plan_create; 0 =
                         never) is cut into segments of that length, one wave each, whose partial sums are stored and added
                         in ascending order -- no atomics: the same bits on every run -- at the price of
                         (2 nnz / 4096 + 1) * (2 * rank * element size + 32) bytes of workspace. */
} skf_theta_desc;

typedef struct {
    int32_t dtype;       /* SKF_F64 / SKF_F32 / SKF_BF16 */
    int32_t variant;     /* SKF_DFMF / SKF_DFMC / SKF_TRANSFORM */
    int32_t target_type; /* SKF_TRANSFORM: the type whose factor is folded in */
    int32_t engine;      /* SKF_ENGINE_MFMA (default) / SKF_ENGINE_VALU */
    /* Row-block sharding only (plans whose relations carry row blocks): this process is part
     * `part_index` of `part_count`; it adds the type-level terms E_i += G_i * sum_r B_r^-,
     * D_i += G_i * sum_r B_r^+ (_dfmf.py:260-264,272-276,278-282 summed over the relations, which is
     * linear in B) on its 1/part_count share of the rows of every type.  0, 0 = all rows. */
    int32_t part_index, part_count;
    int32_t flags;       /* SKF_OPT_* (ABI version 4: the field is new; callers check skf_abi_version() when they load the library) */
} skf_options;

enum {
    SKF_OPT_OWNED_ROWS = 1,/* Ownership-aligned row sharding of ONE fit over `part_count` processes (replaces the
                              reference's per-block joblib tasks, _dfmf.py:69-73, _dfmc.py:341-345): process `part_index` OWNS the
                              rows skf_owned_rows() names of EVERY object type -- their factor rows, their E / D accumulators,
                              their update -- and holds exactly those rows of every relation whose row type it is (the
                              descriptors carry that block, or SKF_REL_ABSENT where the process owns no row of the type), and
                              every constraint in full.  Row-side terms, type-level terms and constraint rows then need NO
                              exchange; per iteration a process sends only: the partial Q = R_blk^T G_i[blk] of every relation
                              (reduce-scatter to the owners of the column type), the updated factor rows (all-gather; SKF_BF16:
                              the bf16 operand copy only, unless a constraint on the type reads the f32 rows), and the c x c
                              partial Gram / W matrices (all-reduce).  Such a plan iterates through skf_iterate_dist only.
                              (Every constraint in full: the dense-fed forms.  One given as its entries is held as the owned
                              rows only, see SKF_OPT_THETA_OWNED_ROWS.) */
    SKF_OPT_THETA_OWNED_ROWS = 2 /* only together with SKF_OPT_OWNED_ROWS (otherwise SKF_E_INVALID): a constraint whose
                              skf_theta_desc.data is NULL is accepted and carries the rows [begin, begin + count) of its type
                              that this process owns (skf_owned_rows) over ALL columns -- the rows the constraint pass of an
                              owned plan multiplies; nothing else of Theta is ever read.  skf_theta_desc.nnz is the entry count
                              of that slice, skf_plan_set_constraint_entries receives indptr[count + 1] rebased to 0; columns
                              stay global.  The lists are those of the whole-matrix form cut at the row boundaries (hub rows
                              are segmented per row from the row's first entry), so the fit has the bits of the fit whose
                              constraint is handed over dense and compacted.  Dense-fed constraints of the same plan are
                              untouched; without the flag a NULL data pointer stays an error on such a plan. */
};

/* ---- plan life cycle ------------------------------------------------------------------- */

/* Validates the graph (shape consistency is a hard error here; the reference only logs it,
 * _dfmf.py:117-123) and builds the per-iteration launch schedule. */
int skf_plan_create(int32_t n_types, const skf_type_desc* types, int32_t n_relations,
                    const skf_relation_desc* relations, int32_t n_thetas,
                    const skf_theta_desc* thetas, const skf_options* options, skf_plan** out);
int skf_plan_destroy(skf_plan* plan);

int skf_plan_workspace_bytes(const skf_plan* plan, size_t* bytes);
/* The known entries of relation `rel` (flagged SKF_REL_KNOWN_CSR; or the stored entries of one flagged SKF_REL_SPARSE_CSR
 * or SKF_REL_FOLD_CSR -- the latter compressed along the target's side, see the flag --, whose values are of the master
 * type -- SKF_BF16: f32), as device pointers: indptr[n_row + 1] (int64; n_row = the LOCAL rows: all of them, or the owned
 * rows of a SKF_OPT_OWNED_ROWS plan, whose slice is rebased to start at 0; a SKF_REL_ABSENT relation takes no call: SKF_E_INVALID;
 * indptr[0] = 0, indptr[n_row] = known_bound, non-decreasing), indices[known_bound] (int32 columns, strictly ascending
 * within a row: canonical CSR, duplicates summed beforehand) and values[known_bound] of the element type of
 * skf_relation_desc.data (SKF_BF16: bf16 bits).  Call it between skf_plan_create and skf_plan_bind_workspace; the buffers
 * are read by skf_plan_bind_workspace and not referenced afterwards (the contract of `data`).  Bind validates them on the
 * device before anything gathers through them: a non-monotone indptr, an index outside [0, n_col) or a row whose
 * columns do not ascend strictly is SKF_E_INVALID, as is a SKF_REL_KNOWN_CSR / SKF_REL_SPARSE_CSR relation without this call. */
int skf_plan_set_known_entries(skf_plan* plan, int32_t rel, const int64_t* indptr, const int32_t* indices,
                               const void* values);
/* The fill vectors of relation `rel` (flagged SKF_REL_FILL_RANK1), as device pointers: row_fill[n_i] = a and col_fill[n_j] = b
 * in the MASTER type (f64 / f32; SKF_BF16 plans: f32).  Call it between skf_plan_set_known_entries and skf_plan_bind_workspace
 * (afterwards: SKF_E_STATE); the buffers are read by skf_plan_bind_workspace, on its stream, and not referenced afterwards
 * (the contract of `data`; `stream` is reserved).  SKF_E_INVALID: a relation without the flag, a null pointer. */
int skf_plan_set_relation_fill(skf_plan* plan, int32_t rel, const void* row_fill, const void* col_fill, void* stream);
/* The stored entries of constraint `theta` (the index into the `thetas` of skf_plan_create; one whose skf_theta_desc.data is
 * NULL, _dfmf.py:284-292 on the dense expansion), as device pointers: indptr[n_i + 1] (int64, indptr[0] = 0,
 * indptr[n_i] = nnz, non-decreasing), indices[nnz] (int32 columns, strictly ascending within a row: canonical CSR, duplicates
 * summed beforehand) and values[nnz] in the MASTER type (f64 / f32; SKF_BF16 plans: f32).  SKF_OPT_THETA_OWNED_ROWS plans:
 * the slice of the owned rows -- indptr[count + 1] rebased to 0 (count = 0: the one pointer 0), indptr[count] = nnz, columns
 * global in [0, n_i); every process makes the call, also one that owns no row.  Call it between skf_plan_create
 * and skf_plan_bind_workspace (afterwards: SKF_E_STATE); the buffers are read by skf_plan_bind_workspace and not referenced
 * afterwards (the contract of `data`).  Bind validates them on the device before anything gathers through them: an indptr
 * that does not run from 0 to nnz or steps down, an index outside [0, n_i) or a row whose columns do not ascend strictly is
 * SKF_E_INVALID with a message naming the constraint, as is such a constraint without this call. */
int skf_plan_set_constraint_entries(skf_plan* plan, int32_t theta, const int64_t* indptr, const int32_t* indices,
                                    const void* values);
/* `workspace` must be 256-byte aligned device memory and stay valid for the plan's lifetime.
 * For DFMC the masked relations are copied into the workspace here (the caller's relation
 * data is never written: _dfmc.py:268, tests/test_dfmc.py:62,85). */
int skf_plan_bind_workspace(skf_plan* plan, void* workspace, size_t bytes, void* stream);

/* ---- factors --------------------------------------------------------------------------- */

/* Precision model: the n-sized matrices (relations, factors G, accumulators E/D, P, Q) live in
 * the master type -- f64 for SKF_F64, f32 otherwise.  Every c x c matrix (Gram, its
 * pseudo-inverse, backbones S and the B/D terms) is kept and combined in f64 in ALL engines, and
 * the two reductions over the object dimension that feed them (G^T G, G^T P) accumulate in f64:
 * the Gram matrices of real data are ill-conditioned (cond ~1e5 for the reference's dicty
 * example) and an all-f32 pipeline diverges where the f64 reference does not.
 * set_factor copies an n_obj x rank matrix in  set_factor copies an n_obj x rank matrix in
 * (the G0 of `initialize`, _init.py:6-61, or a frozen fitted factor for SKF_TRANSFORM). */
int skf_set_factor(skf_plan* plan, int32_t type, const void* G, int64_t ld, void* stream);
int skf_get_factor(const skf_plan* plan, int32_t type, void* G, int64_t ld, void* stream);
/* backbone S of relation `rel` (rank_row x rank_col).  set: SKF_TRANSFORM only (frozen S). */
int skf_set_backbone(skf_plan* plan, int32_t rel, const void* S, int64_t ld, void* stream);
int skf_get_backbone(const skf_plan* plan, int32_t rel, void* S, int64_t ld, void* stream);

/* ---- the hot path ---------------------------------------------------------------------- */

/* Runs `n_iters` full update iterations (the body of `for iter in range(max_iter)`,
 * _dfmf.py:212-296 / _dfmc.py:270-366 / _dfmf.py:370-428) device-resident on `stream`.
 * After the call get_backbone returns the S computed from the factors BEFORE the last G update
 * and get_factor the factors AFTER it -- the same generation mismatch the reference returns
 * (_dfmf.py:239 vs :295, return :327). */
int skf_iterate(skf_plan* plan, int32_t n_iters, void* stream);
/* The same for `n_plans` (1 .. 64) plans of ONE graph at once -- independent random restarts (the reference's n_run loop
 * over joblib workers, dfmf.py:87-95) of a graph too small to fill the chip: every launch of the iteration serves all of
 * them (the restart is a grid dimension), so ten restarts of the dicty graph cost little more than one.  The plans must
 * have been created from the same object types, ranks, relation shapes and engine and must run the schedule for small
 * graphs (SKF_DFMF, every rank <= 64, sparse constraints, at most 8192 objects per type); each keeps its own workspace,
 * factors and results, exactly as after skf_iterate.  SKF_E_STATE when the plans do not batch: iterate them one by one.
 * SKF_TRANSFORM plans batch as well: the fold-ins of ONE set of new relations into the models of several restarts (the
 * reference's n_run fold-ins over joblib workers, dfmf.py:191-199) -- same object types, ranks and relations, each plan with
 * the frozen factors / backbones of its restart, no constraint on the target type; one launch per iteration serves all. */
int skf_iterate_batch(skf_plan* const* plans, int32_t n_plans, int32_t n_iters, void* stream);
/* *yes = 1 when the (bound) plan can be one of the plans of skf_iterate_batch: the schedule for small graphs, or a fold-in
 * without constraints on the target type. */
int skf_plan_batchable(const skf_plan* plan, int32_t* yes);
/* The limits behind that verdict for SKF_DFMF plans in f32 / f64 (the three-launch schedule of small graphs): every rank
 * <= *max_rank, every type <= *max_objects objects, at most *max_types / *max_relations / *max_constraints of each, every
 * constraint sparse (0 < nnz <= n * n / *constraint_nnz_divisor), no masked, absent or row-block relation -- so that a host
 * layer can decide whether restarts will share launches WITHOUT uploading the graph (the reference hands restarts to joblib
 * workers, dfmf.py:87-95; here the host picks between skf_iterate_batch and one plan after the other).  Null pointers are
 * skipped. */
int skf_small_graph_limits(int32_t* max_rank, int64_t* max_objects, int32_t* max_types, int32_t* max_relations,
                           int32_t* max_constraints, int32_t* constraint_nnz_divisor);
/* enable != 0: iterations 2..n of skf_iterate replay ONE captured hipGraph (a single host call per
 * iteration instead of one per kernel).  Off by default -- a single fit is bound by kernel time --
 * and switched on for restarts that run CONCURRENTLY on several streams of one GPU, where the
 * host-side launch rate of one thread is the limit (the reference's n_jobs over n_run restarts,
 * dfmf.py:87-95).  A failed capture falls back to eager launches. */
int skf_plan_set_graph(skf_plan* plan, int32_t enable);

/* The same iteration in two halves, for runs whose relations are partitioned over several GPUs
 * (one process and one plan per GPU, each plan holding ALL object types but only its share of
 * the relations / constraints; factors replicated):
 *     skf_accumulate   : Gram, pinv, contractions, backbones and the E / D accumulator sums of
 *                        the plan's own relations and constraints
 *     <all-reduce(sum) of the accumulator range over the ranks -- RCCL via torch.distributed>
 *     skf_apply_update : G <- G * sqrt(E / max(D, eps))          (identical on every rank)
 * skf_accumulator_range reports the byte range [offset, offset+bytes) of the workspace that
 * holds every E and D matrix (master dtype; padding between slots is zero-safe to reduce). */
int skf_accumulate(skf_plan* plan, void* stream);
int skf_apply_update(skf_plan* plan, void* stream);
int skf_accumulator_range(const skf_plan* plan, size_t* offset, size_t* bytes);

/* Row-block sharding: every process creates a plan with ALL object types and ALL relations, each
 * relation carrying this process's row block (or SKF_REL_ABSENT); exactly one holder per relation
 * leaves SKF_REL_NO_COL_SIDE clear.  One iteration is then four stages with an all-reduce(sum)
 * over the processes of a workspace byte range between them (skf_exchange_range; the ranges have
 * the same layout in every such plan):
 *     skf_stage(SKF_STAGE_CONTRACT)    Gram, pinv, local P = R_blk G_j, partial Q = R_blk^T G_i[blk],
 *                                      partial W = G_i[blk]^T P          -> reduce SKF_X_W, SKF_X_Q
 *     skf_stage(SKF_STAGE_BACKBONE)    S = K_i W K_j; DFMC: completion of the local rows, P and
 *                                      partial Q of masked relations     -> reduce SKF_X_QM (DFMC)
 *     skf_stage(SKF_STAGE_ACCUMULATE)  E / D terms of the local rows, column-side and Theta terms
 *                                                                        -> reduce SKF_X_ED
 *     skf_stage(SKF_STAGE_UPDATE)      G <- G * sqrt(E / max(D, eps))
 * (the +- split of _dfmf.py:256-276 is non-linear, hence Q is reduced raw, before it).
 * skf_accumulate == the first three stages back to back (plans without row blocks);
 * skf_iterate refuses a plan with row blocks.  skf_relation_sqerr covers the local rows. */
enum { SKF_STAGE_CONTRACT = 0, SKF_STAGE_BACKBONE = 1, SKF_STAGE_ACCUMULATE = 2, SKF_STAGE_UPDATE = 3 };
enum { SKF_X_W = 0, SKF_X_Q = 1, SKF_X_QM = 2, SKF_X_ED = 3 };
int skf_stage(skf_plan* plan, int32_t stage, void* stream);
/* dtype: SKF_F64 for SKF_X_W, the master type otherwise; bytes may be 0 (nothing to reduce). */
int skf_exchange_range(const skf_plan* plan, int32_t which, size_t* offset, size_t* bytes, int32_t* dtype);

/* ---- collectives behind the boundary ------------------------------------------------------------------------------
 * The reference spreads its restarts over joblib workers (dfmf.py:87-95) and its block products over `_par_bdot`
 * (_dfmf.py:69-73); a fit spread over several GPUs needs the sums of the E / D accumulators (and, with row blocks, of W
 * and Q) instead.  A communicator is either RCCL -- bound with dlopen at run time (the librccl of the process if one is
 * loaded, else SKF_RCCL_PATH / the loader path / /opt/rocm/lib), one process per GPU, the current device at
 * skf_comm_create -- or a callback the caller supplies (another transport; the CPU tests run it over gloo).
 *     rank 0: skf_comm_unique_id(id)  -> hand the 128 bytes to every rank ->  skf_comm_create(id, rank, world, &comm)
 *     skf_plan_set_comm(plan, comm);  skf_iterate_dist(plan, n_iters, stream)
 * skf_iterate_dist = the same iteration as skf_accumulate + all-reduce + skf_apply_update (plans without row blocks) or the
 * four skf_stage calls with their exchanges (plans with row blocks), issued on `stream` by the library itself: W, Q as
 * all-reduce; E and D as REDUCE-SCATTER over `world` equal element ranges of the accumulator regions, the multiplicative
 * update of the owned range of G, and an ALL-GATHER of G -- 3 (world-1)/world of the factor bytes per rank and iteration
 * instead of the 4 (world-1)/world of all-reducing both accumulators (config 3 on 8 GPUs: 444 MB instead of 592 MB).  Every
 * rank ends an iteration with identical factors.  skf_exchange_bytes: bytes one rank sends per iteration on a ring.
 * SKF_OPT_OWNED_ROWS plans (ownership-aligned row blocks): no exchange of E / D at all -- all-reduce of the c x c partial
 * Gram and W matrices, one reduce-scatter per relation of its partial Q to the owners of the column type, update of the
 * OWNED rows, one all-gather per type of the updated rows (SKF_BF16: of their bf16 operand copy; the f32 rows of the other
 * owners are fetched once, at the end of the call).  The exchanges go out on a stream of their own as soon as their input
 * is complete -- a relation's Q under the next relation's contractions, a type's gather as soon as its last relation is
 * through -- and the communicator's (rank, world) must be the plan's (part_index, part_count).  Config 3 on 8 GPUs, bf16:
 * 172 MB per rank and iteration instead of 605 MB. */
typedef struct skf_comm skf_comm;
/* op 0: all-reduce(sum) of `count` elements in place; 1: reduce-scatter(sum) -- `buf` holds world * count elements, on
 * return elements [rank * count, (rank + 1) * count) are reduced; 2: all-gather of that range to every rank, in place.
 * dtype SKF_F64 / SKF_F32 (SKF_BF16: 2-byte elements, all-gather only); `buf` is device memory, the call is ordered on
 * `stream`; return 0 on success. */
typedef int (*skf_collective_fn)(void* user, int32_t op, void* buf, size_t count, int32_t dtype, void* stream);
int skf_comm_unique_id(void* id128);
int skf_comm_create(const void* id128, int32_t rank, int32_t world, skf_comm** out);   /* id128 == NULL: world must be 1 */
int skf_comm_create_callback(int32_t rank, int32_t world, skf_collective_fn fn, void* user, skf_comm** out);
/* A communicator that exchanges nothing: `rank` of `world` on ONE device, for timing the compute of that rank of a
 * sharded fit where the other ranks do not exist (bench.py --emulate-rank k/W).  A sum over the ranks is stood in for by
 * world x this rank's partial sum and the multiplicative update of the owned rows is not applied (so that the Gram matrices
 * the timed launches see stay those of well-conditioned factors and the pseudo-inverses take the path they take in a real
 * run); gathers leave the other ranks' rows as they were.  Every other launch of the iteration runs. */
int skf_comm_create_null(int32_t rank, int32_t world, skf_comm** out);
/* What a communicator is: its rank / world as created, its transport, and how many ranks the transport itself reports
 * (SKF_COMM_RCCL: ncclCommCount of the bound communicator, -1 when the library does not export it; callback: world;
 * single: 1; null: 0) -- lets a caller (bench.py's strong-scaling record) state that RCCL really spans the ranks of the
 * run.  Null pointers are skipped. */
enum { SKF_COMM_SINGLE = 0, SKF_COMM_RCCL = 1, SKF_COMM_CALLBACK = 2, SKF_COMM_NULL = 3 };
int skf_comm_info(const skf_comm* comm, int32_t* rank, int32_t* world, int32_t* transport, int32_t* transport_ranks);
int skf_comm_destroy(skf_comm* comm);
int skf_plan_set_comm(skf_plan* plan, skf_comm* comm);     /* not owned by the plan; NULL detaches */
int skf_iterate_dist(skf_plan* plan, int32_t n_iters, void* stream);
int skf_exchange_bytes(const skf_plan* plan, int32_t world, size_t* bytes);

/* sum over the relation of (R - G_i S G_j^T)^2 with the current (G, S), written as one f64 to
 * the DEVICE address `out` (reconstruction error of _dfmf.py:306-316 without materialising the
 * n_i x n_j product).  For DFMC the working copy (completed entries) is used.  SKF_BF16: one pass
 * over the stored bf16 relation, bf16-rounded G_i S and G_j on the matrix cores, f32 residual.
 * A SKF_REL_SPARSE_CSR relation: tr(S^T Gram_i S Gram_j) from c x c f64 products plus one pass over the row lists,
 * sum of (r - x)^2 - x^2 with x = <(G_i S)[row], G_j[col]> in the master type (SKF_BF16: the f32 masters, not the bf16
 * rows), f64 partials per wave summed in a fixed order.  A SKF_REL_FOLD_CSR relation: the same, over its one set of lists.
 * A SKF_REL_FOLD_CSR | SKF_REL_FOLD_KNOWN relation: the KNOWN-ENTRY objective, sum over the stored entries of (v - x)^2 with
 * x = <G_t[o], T[i]> and the current target factor, in the master type -- one pass over the lists, f64 partials per wave
 * summed in a fixed order.  This is NOT the reference's norm of the working copy, which carries the PREVIOUS iterate in the
 * unknown cells (_dfmc.py:376-389): no previous iterate is kept here. */
int skf_relation_sqerr(skf_plan* plan, int32_t rel, double* out, void* stream);

/* The two contraction results the LAST iteration left in the workspace, for verification at sizes where the
 * host cannot recompute them: which = 0: P = R G_j (local rows x rank_col), 1: Q = R^T G_i (n_col x rank_row),
 * both from the factors BEFORE that iteration's update (like the backbone), master dtype, copied to `dst`.
 * A masked relation kept as known entries only (skf_relation_desc.known_bound) never forms P: it answers
 * which = 2 with the row-side product P S^T (n_row x rank_row) it computes instead, and which = 1 as usual.
 * A SKF_REL_FOLD_CSR relation forms neither: SKF_E_INVALID. */
int skf_get_contraction(const skf_plan* plan, int32_t rel, int32_t which, void* dst, int64_t ld, void* stream);

/* The entry lists a relation keeps after bind (a masked relation kept as its known entries, a SKF_REL_KNOWN_CSR or a
 * SKF_REL_SPARSE_CSR relation), for verification: by_col = 0 the row lists (rows -> ascending columns), 1 the column lists
 * (columns -> ascending rows).  `parts` / `n_entries` (host) receive the number of parts the lists are cut into and the
 * number of entries; `ptr` (device, n * parts + 1 int64: the segment pointers, every `parts`-th one opens a list), `idx`
 * (device, n_entries int32) and `values` (device, n_entries of the master type) receive copies.  Null pointers are skipped.
 * A SKF_REL_FILL_RANK1 relation: `values` are d = v - a_r b_c, what the passes multiply, not the stored values v.
 * SKF_OPT_OWNED_ROWS plans: the lists of the slice -- n = the local rows for the row lists, and the column lists hold LOCAL row
 * indices (row - row_begin); SKF_E_STATE for a SKF_REL_ABSENT relation. */
int skf_get_relation_lists(const skf_plan* plan, int32_t rel, int32_t by_col, int32_t* parts, int64_t* n_entries, int64_t* ptr,
                           int32_t* idx, void* values, void* stream);

/* The lists a constraint keeps after bind, for verification: one handed over dense and compacted (skf_theta_desc.nnz > 0),
 * one given as its entries, or the slice of the owned rows of a SKF_OPT_THETA_OWNED_ROWS plan.  `n_rows` / `n_entries` (host)
 * receive the rows the lists cover (n_i, or the owned rows of the slice) and the number of entries; `indptr` (device,
 * n_rows + 1 int64), `indices` (device, n_entries int32) and `values` (device, n_entries of the master type) receive copies.
 * Null pointers are skipped.  SKF_E_INVALID for a constraint kept dense. */
int skf_get_constraint_lists(const skf_plan* plan, int32_t theta, int64_t* n_rows, int64_t* n_entries, int64_t* indptr,
                             int32_t* indices, void* values, void* stream);

/* Optional hipEvent timing of the launches that walk a relation (P = R G_j, Q = R^T G_i -- the dominant
 * kernel -- and their sparse counterparts).  get_profile synchronises on the recorded events, returns the summed
 * duration [ms], the number of launches, the flops they EXECUTE (2*M*N*K for a product on the matrix cores, dense or
 * bitmap; 2 * ones * N for the row gathers of a very sparse 0/1 relation; 2 or 4 * known * c for a pass over the
 * known entries of a masked relation; 2 * stored * N for a pass over a SKF_REL_SPARSE_CSR relation, whose bytes are its
 * index + value lists and the factor rows it gathers) and the relation bytes they read from HBM as stored (bf16 / f32 / f64 entries,
 * 1 bit per entry for a bitmap, index + value lists for the sparse forms) since the last call, and resets the counters.
 * A SKF_REL_FILL_RANK1 relation adds, per pass, ONE launch (the weighted column sum of the gathered factor with its reduce;
 * the rank-one term rides the launch that sums the parts), 2 n_in w + 2 n_out w flops (n_in rows of the gathered factor, w its
 * rank, n_out rows of the output) and n_in (w g + e) + n_out e bytes (g = bytes of a gathered element, e of a master one: the
 * factor with its weights, the scale vector), plus 2 n_out w e where the lists have one part (the output read and written
 * once more). */
int skf_plan_set_profiling(skf_plan* plan, int32_t enable);
int skf_plan_get_profile(skf_plan* plan, double* total_ms, int64_t* launches, double* flops, double* bytes);

/* ---- stand-alone operators (building blocks, exported for tests / callers) -------------- */

typedef struct {
    const void* A; /* A(m,k) = A[m*sa_m + k*sa_k] */
    const void* B; /* B(k,n) = B[k*sb_k + n*sb_n] */
    void* C;
    void* C2;
    const uint8_t* mask;
    int64_t sa_m, sa_k, sb_k, sb_n, ldc, ldc2, ldmask;
    int32_t M, N, K;
    int32_t aop;        /* 0: x   1: max(x,0)   2: max(-x,0)  applied to A on load */
    int32_t epi;        /* 0 store, 1 accumulate, 2 split-store, 3 split-accumulate, 4 masked store */
    int32_t nan_to_num; /* numpy.nan_to_num on the product before the epilogue */
    int32_t splits;     /* 0 = choose; >1 needs workspace of splits*M*N elements */
    int32_t a_dtype;    /* storage type of A / B: -1 = same as `dtype`, else SKF_F64 / SKF_F32.   */
    int32_t b_dtype;    /* supported (C,A,B): (f64,f64,f64) (f32,f32,f32) (f64,f32,f32) (f32,f32,f64) */
} skf_gemm_desc;

/* C = epi(aop(A) * B) on the matrix cores; `dtype` = arithmetic and result type (f64 / f32). */
int skf_gemm(int32_t dtype, int32_t engine, const skf_gemm_desc* desc, void* workspace,
             size_t workspace_bytes, void* stream);

/* bf16 relation contraction C[M x N] (f32) = A[M x Kp] * Bt[N x Kp]^T, both operands bf16,
 * row-major and K-contiguous, Kp a multiple of 64 with zero-filled padding, lda/ldb multiples of
 * 8 and 16-byte aligned bases (v_mfma_f32_16x16x32_bf16, f32 accumulation).  `splits` = 0 lets
 * the library choose the K slicing; >1 needs a workspace of splits*M*N floats. */
int skf_gemm_bf16(const void* A, int64_t lda, const void* Bt, int64_t ldb, float* C, int64_t ldc,
                  int32_t M, int32_t N, int32_t Kp, int32_t splits, void* workspace,
                  size_t workspace_bytes, void* stream);

/* The transposed-A form of the same contraction, C[M x N] (f32) = A[Kp x M]^T * Bt[N x Kp]^T: A is
 * row-major [Kp][lda] with the OUTPUT rows along its columns (lda >= M, lda % 8 == 0, rows zero-filled
 * up to Kp % 64 == 0).  This is Q = R^T G_i read from the row-major relation itself: the A tile lands in
 * LDS as stored and the fragments are read transposed (ds_read_b64_tr_b16) -- no stored R^T
 * (reference _dfmf.py:266 multiplies the strided view R.T the same way, without a copy). */
int skf_gemm_bf16_tn(const void* A, int64_t lda, const void* Bt, int64_t ldb, float* C, int64_t ldc,
                     int32_t M, int32_t N, int32_t Kp, int32_t splits, void* workspace,
                     size_t workspace_bytes, void* stream);

/* The same two contractions with a BINARY A operand stored as a bitmap (SKF_REL_BINARY): bit (c & 7) of byte
 * A[r * lda_bytes + (c >> 3)] is entry (r, c), lda_bytes a multiple of 8, padding bits zero.
 * transposed == 0: C[M x N] = A[M x Kp] * Bt^T (rows of the bitmap = output rows);
 * transposed != 0: C[M x N] = A[Kp x M]^T * Bt^T (rows of the bitmap = the contraction index, zero rows up to Kp). */
int skf_gemm_bits(const void* A, int64_t lda_bytes, const void* Bt, int64_t ldb, float* C, int64_t ldc,
                  int32_t M, int32_t N, int32_t Kp, int32_t transposed, int32_t splits, void* workspace,
                  size_t workspace_bytes, void* stream);

/* dst (bf16, ld ldd) = round-to-nearest-even(src) or its transpose; src dtype SKF_F64 / SKF_F32 /
 * SKF_BF16.  Padding columns of dst are left untouched (zero them beforehand).  SKF_F64 is rounded to f32 first (two
 * roundings, as the host's to_bf16_bits: at most 2^-17 bf16 ulp from one); a NaN becomes a quiet NaN of the same sign; a
 * bf16 source is copied.  SKF_E_INVALID for lds < cols and for ldd below a row of dst (cols; rows when transposed). */
int skf_to_bf16(void* dst, int64_t ldd, int32_t src_dtype, const void* src, int64_t lds,
                int64_t rows, int64_t cols, int32_t transpose, void* stream);

/* Ec[o][q] += max(x, 0), Dc[o][q] += max(-x, 0) with x = sum over the list of output object o, in LIST ORDER, of
 * fma(values[k], T[indices[k]][q], x), for o < n_out and q < c (1 .. 1024): the constant numerator / denominator sums of a
 * fold-in through a sparse relation (reference _dfmf.py:394-398,408-412: tmp1 = R G_j S^T resp. R^T G_i S split into its
 * positive and negative part) on the caller's buffers.  dtype SKF_F64 / SKF_F32 is the type of values, T, Ec and Dc;
 * indptr[n_out + 1] (int64) and indices (int32 rows of T) are not validated here (skf_plan_bind_workspace validates the
 * lists of a SKF_REL_FOLD_CSR relation before this pass runs over them).  Every (o, q) is owned by one lane: no atomics, no
 * cross-lane sum -- the result is the host loop's, bit for bit.  Memory past column c of a row is not touched. */
int skf_fold_lists(int32_t dtype, const int64_t* indptr, const int32_t* indices, const void* values, int64_t n_out,
                   const void* T, int64_t ldt, int32_t c, void* Ec, int64_t lde, void* Dc, int64_t ldd, void* stream);

/* One iteration's pass of a fold-in on KNOWN entries (SKF_REL_FOLD_KNOWN) on the caller's buffers: for o < n_out, q < c
 * (1 .. 1024), with the list (i_k, v_k) of output object o
 *     tmp1[o][q] = X[o][q] + sum_k (v_k - <G[o], T[i_k]>) T[i_k][q] ,  E[o][q] += max(tmp1, 0) ,  D[o][q] += max(-tmp1, 0)
 * X (n_out x c, the caller's G B) may be NULL: nothing is added (ldx is then ignored).  dtype SKF_F64 / SKF_F32 is the type
 * of values, G, T, X, E and D.  Arithmetic order: `lanes` = the smallest power of two >= min(c, 64) lanes share an object, lane
 * l owns the columns l, l + lanes, ...; the prediction is part_l = fma(G[o][q], T[i_k][q], part_l) over the lane's columns
 * in ascending order, then the xor butterfly part += part of lane (l ^ off) for off = 1, 2, 4, ... < lanes; e = v_k - x;
 * acc[q] = fma(e, T[i_k][q], acc[q]) in LIST ORDER; tmp1 = acc[q] + X[o][q].  Every (o, q) has one owner: no atomics, the same
 * bits on every run.  An object with an empty list gets tmp1 = X[o].  Validation as for skf_fold_lists (the lists themselves
 * are not validated here: skf_plan_bind_workspace does that for a plan's).  Memory past column c of a row is not touched. */
int skf_fold_known_pass(int32_t dtype, const int64_t* indptr, const int32_t* indices, const void* values, int64_t n_out,
                        const void* G, int64_t ldg, const void* T, int64_t ldt, int32_t c, const void* X, int64_t ldx, void* E,
                        int64_t lde, void* D, int64_t ldd, void* stream);

/* The k best columns of every row of X = H Gc^T, H = G_row[rows] S (m x c, formed by the caller with skf_gemm), Gc = G_col
 * (n_cols x c), without X: the reference materialises X on the host (fusion/base/base.py `complete`: np.dot(G1, np.dot(S,
 * G2.T))) and its users rank or index that array (examples/movielens_completion.py:121-126).  Score tiles are formed on the
 * matrix cores and selected on the compute unit; nothing of size m x n_cols is written anywhere.
 *   Order: higher score first, equal scores by lower column; a NaN score is never selected.  score(r, j) is summed in the
 *     same order whatever the tile, col_splits or launch geometry: the output is bit-identical for every col_splits.
 *   Exclusion (optional; both pointers NULL = none): CSR over the m rows, excl_indptr[m + 1] (int64, from 0, non-decreasing;
 *     excl_indptr[m] is the number of entries), excl_indices (int32 columns, in range, strictly ascending within a row).  A
 *     listed column is never a candidate.  The lists are validated on the device before the pass; an invalid list is refused
 *     (SKF_E_INVALID, outputs not written), not read out of bounds.
 *   Output: out_idx[r * ld_idx + s] (int32) and out_val[r * ld_val + s] (dtype), s < k, best first; slots no candidate fills
 *     hold -1 and -inf.
 *   col_splits: the column range is cut into that many parts (each a whole number of 64-column tiles, at most 32 parts and
 *     never more than there are tiles), one workgroup per (64 rows, part), merged by a second kernel under the same order;
 *     0 = the library chooses (few rows still fill the chip).  skf_complete_topk_workspace_bytes with the same m, n_cols, k
 *     and col_splits sizes the workspace (256-byte aligned; 0 sizes for what the launch will choose).
 *   dtype SKF_F64 / SKF_F32 (the type of H, Gc and out_val); 1 <= c <= 1024, 1 <= k <= SKF_TOPK_MAX, m and n_cols < 2^31. */
#define SKF_TOPK_MAX 64
int skf_complete_topk_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int32_t k, int32_t col_splits, size_t* bytes);
int skf_complete_topk(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols,
                      int32_t c, int32_t k, const int64_t* excl_indptr, const int32_t* excl_indices,
                      int32_t* out_idx, int64_t ld_idx, void* out_val, int64_t ld_val,
                      int32_t col_splits /* 0 = choose */, void* workspace, size_t workspace_bytes, void* stream);

/* out[e] = sum over q < c of H[rows[e]][q] * Gc[cols[e]][q] for e < n: the predictions at given pairs (what the reference
 * reads as R12_pred[hidden] from the dense product, examples/movielens_completion.py:121-126).  rows (int32, into the m rows
 * of H) and cols (int32, into the n_cols rows of Gc) are checked on the device before the pass: an index out of range gives
 * SKF_E_INVALID and leaves out as it was.  16 adjacent lanes share an entry and fold their partial sums in a fixed order:
 * two runs give the same bits.  dtype SKF_F64 / SKF_F32; 1 <= c <= 1024. */
int skf_complete_entries(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols,
                         int32_t c, const int32_t* rows, const int32_t* cols, int64_t n, void* out, void* stream);

/* The rank of given (row, column) pairs in X = H Gc^T (H, Gc as for skf_complete_topk) without X: the one number per
 * held-out pair that Recall@k, MRR, NDCG and AUC need of the array the reference's users rank
 * (examples/movielens_completion.py:121-126).  For a target (r, j) with s = score(r, j):
 *     rank(r, j) = #{ j' in [0, n_cols), j' != j, j' not in row r's exclusion list, score(r, j') not NaN,
 *                     score(r, j') > s  or  (score(r, j') == s and j' < j) }
 *   -- the 0-based position of j in the total order of skf_complete_topk: higher score first, equal scores by lower column,
 *   NaN never.  A target with a NaN score gets -1.  A target that is itself in the exclusion list is still ranked: exclusion
 *   removes competitors only.  score(r, j) is the same chain of matrix instructions as in skf_complete_topk, hence
 *   P1: if (r, j) is not excluded and rank(r, j) = p < k <= 64, skf_complete_topk on the same inputs returns
 *     out_idx[r][p] == j and out_val[r][p] with the bits of out_val[e]; if p >= k, j is not in row r's list -- for every
 *     col_splits of either operator.
 *   Targets: CSR over the m rows, tgt_indptr[m + 1] (int64, from 0, non-decreasing, tgt_indptr[m] == n_targets),
 *     tgt_indices (int32 columns, in range, strictly ascending within a row).  Exclusion: as for skf_complete_topk (both
 *     pointers NULL = none).  Both lists are validated on the device before anything gathers through them; an invalid list
 *     gives SKF_E_INVALID and leaves out_rank and out_val as they were.
 *   Output: out_rank[e] (int32) and, unless NULL, out_val[e] = score of target e (dtype), e < n_targets in list order.
 *   Counts are integers added with integer atomics: the result does not depend on col_splits (0 = the library chooses, at
 *     most 32) or the launch geometry.  skf_complete_ranks_workspace_bytes sizes the workspace (256-byte aligned): flag
 *     words and n_targets scores, nothing that grows with m x n_cols.  n_targets == 0 succeeds without a launch.
 *   dtype SKF_F64 / SKF_F32; 1 <= c <= 1024; m and n_cols < 2^31. */
int skf_complete_ranks_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int64_t n_targets, int32_t col_splits,
                                       size_t* bytes);
int skf_complete_ranks(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols,
                       int32_t c, const int64_t* tgt_indptr, const int32_t* tgt_indices, int64_t n_targets,
                       const int64_t* excl_indptr, const int32_t* excl_indices, int32_t* out_rank,
                       void* out_val /* dtype, may be NULL */, int32_t col_splits /* 0 = choose */, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Every pair of X = H Gc^T (H, Gc as for skf_complete_topk) that scores at or above a per-row threshold, as a sparse matrix
 * and without X: link prediction reads the reference's dense product (fusion/base/base.py `complete`: np.dot(G1, np.dot(S,
 * G2.T))) against a cut-off; here nothing of size m x n_cols is written anywhere.  For row r with threshold thr[r]:
 *     above(r) = { j in [0, n_cols) : j not in row r's exclusion list, score(r, j) >= thr[r] }
 *   score(r, j) is the same chain of matrix instructions as in skf_complete_topk and >= is the IEEE comparison: a NaN score
 *   or a NaN threshold selects nothing, -inf selects every admissible column whose score is not NaN, +inf only +inf scores.
 *   Output: canonical CSR over the m rows -- out_indptr[m + 1] (int64, from 0), out_indices (int32, strictly ascending within
 *     a row) and, unless NULL, out_values (dtype, the scores).  The pass runs twice over the tiles (count, integer scan,
 *     fill); the position of every entry is a function of the inputs alone, so the bytes are the same for every col_splits
 *     (0 = the library chooses, at most 32) and every run.  No atomics on positions, no float atomics.
 *   capacity: entries out_indices (and out_values) can hold.  *n_found (host) is the number of entries found.
 *     out_indices == NULL (out_values then NULL too): count only -- out_indptr and *n_found are written.
 *     *n_found > capacity: SKF_E_WORKSPACE, the message names both numbers; out_indptr and *n_found are written, out_indices
 *       and out_values are not touched -- call again with that capacity.
 *     otherwise: everything is written and the memory behind entry *n_found is not touched.
 *     m == 0 or n_cols == 0: success without a product launch, out_indptr all zero, *n_found = 0.
 *   Exclusion: as for skf_complete_topk (both pointers NULL = none), validated on the device before anything gathers
 *     through the lists.  Every refusal (SKF_E_INVALID; SKF_E_WORKSPACE for a workspace that is NULL, too small or not
 *     256-byte aligned) leaves every output as it was.  skf_complete_above_workspace_bytes sizes the workspace: flag words,
 *     the words of the scan and one int64 per (column split, row), nothing that grows with m x n_cols.
 *   dtype SKF_F64 / SKF_F32 (the type of H, Gc, thr and out_values); 1 <= c <= 1024; m and n_cols < 2^31. */
int skf_complete_above_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int32_t col_splits, size_t* bytes);
int skf_complete_above(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols,
                       int32_t c, const void* thr /* dtype [m], device */,
                       const int64_t* excl_indptr, const int32_t* excl_indices,
                       int64_t capacity, int64_t* out_indptr /* [m + 1], device */,
                       int32_t* out_indices /* [capacity] or NULL */, void* out_values /* dtype [capacity] or NULL */,
                       int64_t* n_found /* host */, int32_t col_splits /* 0 = choose */,
                       void* workspace, size_t workspace_bytes, void* stream);

/* One counting pass of a radix select over EVERY candidate score of X = H Gc^T (H, Gc as for skf_complete_topk), without X:
 * what finds the n-th largest score of a whole relation -- the cut-off of "the n most confident pairs over all rows", which
 * the reference's users read off the sorted dense product (fusion/base/base.py `complete`) -- in KEY_BITS / 11 passes.
 *   Candidate: a pair (r, j), j in [0, n_cols), j not in row r's exclusion list, score(r, j) not NaN; score(r, j) is the same
 *     chain of matrix instructions as in skf_complete_topk.
 *   Key: u = the bits of score + 0 as an unsigned integer of KEY_BITS = 32 (SKF_F32) / 64 (SKF_F64);
 *     key = u ^ (sign bit of u set ? all ones : the sign bit).  key(a) < key(b) <=> a < b; -0.0 and +0.0 share one key;
 *     -inf and +inf are ordinary keys, the smallest and the largest.
 *   Counting: a candidate counts when the top prefix_bits of its key equal prefix; it adds one to
 *     hist[(key >> (KEY_BITS - prefix_bits - digit_bits)) & (2^digit_bits - 1)].  hist (device, uint64 [1 << digit_bits]) is
 *     ADDED to, never cleared: the caller clears it once, sums the row blocks of one pass on the device and reads it back once
 *     per pass.  Integer atomics only: the counts do not depend on col_splits (0 = the library chooses, at most 32), the
 *     launch geometry or the order of arrival.
 *   Selection (the caller's): walk a pass's histogram from the highest digit down to the bin that holds the n-th candidate,
 *     append the digit to the prefix, take the counts above the bin off n, repeat until prefix_bits == KEY_BITS.  Then the
 *     prefix is key(T), T the n-th largest candidate score, g = the candidates > T, e = the last bin = the candidates == T, and
 *   P3: skf_complete_above with thr[r] = T in every row returns exactly g + e entries on the same inputs, g of them > T and e
 *     of them == T, with g < n <= g + e -- for every col_splits and every cut of the rows into blocks of either operator.  For
 *     a single row and n <= 64 the n best pairs are skf_complete_topk's list, index for index and bit for bit.
 *   Refused with SKF_E_INVALID and nothing written: digit_bits outside 1 .. 11, prefix_bits < 0, prefix_bits + digit_bits >
 *     KEY_BITS, prefix >= 2^prefix_bits, hist NULL, the operand checks of skf_complete_topk; SKF_E_WORKSPACE for a workspace
 *     that is NULL, too small or not 256-byte aligned (skf_complete_digits_workspace_bytes: flag words only).  Exclusion: as
 *     for skf_complete_topk (both pointers NULL = none), validated on the device before anything is counted.  m == 0 (or
 *     n_cols == 0) succeeds and adds nothing.
 *   dtype SKF_F64 / SKF_F32; 1 <= c <= 1024; m and n_cols < 2^31. */
int skf_complete_digits_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int32_t col_splits, size_t* bytes);
int skf_complete_digits(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols,
                        int32_t c, const int64_t* excl_indptr, const int32_t* excl_indices,
                        uint64_t prefix, int32_t prefix_bits, int32_t digit_bits,
                        uint64_t* hist /* device, [1 << digit_bits], ADDED to */,
                        int32_t col_splits /* 0 = choose */, void* workspace, size_t workspace_bytes, void* stream);

/* The histogram BY VALUE of every candidate score of X = H Gc^T (H, Gc as for skf_complete_topk) and of the scores of given
 * target pairs, in one walk and without X: how many pairs lie above each of many cut-offs, precision / recall / false-positive
 * rate at those cut-offs against a gold standard, the micro-averaged ROC and PR curves and the AUROC, which the reference's
 * users read from roc_auc_score on the dense product (examples/pharma_chaining.py:100, examples/movielens_completion.py:121-126).
 *   Candidate: as for skf_complete_digits -- j in [0, n_cols), j not in row r's exclusion list, score(r, j) not NaN; score(r, j)
 *     is the same chain of matrix instructions as in skf_complete_topk.
 *   Bin of a candidate score s: bin(s) = #{ t < n_edges : edges[t] <= s }, 0 .. n_edges, with the IEEE comparison in dtype -- the
 *     one skf_complete_above makes: s >= edges[t] <=> bin(s) > t; -0.0 and +0.0 compare equal; -inf and +inf are ordinary
 *     scores and ordinary edges.  edges (device, dtype [n_edges], 1 <= n_edges <= SKF_HIST_MAX_EDGES): none NaN, non-decreasing;
 *     equal neighbours are allowed and give empty bins.
 *   Counting: every candidate adds one to hist[bin]; with targets -- a CSR over the m rows exactly as skf_complete_ranks takes
 *     it, tgt_indptr[m] == n_targets -- a candidate that is a target adds one to hist_tgt[bin] as well: hist counts all
 *     candidates, targets included, and a target that is excluded or scores NaN is no candidate and is counted nowhere.  Both
 *     histograms (device, uint64 [n_edges + 1]) are ADDED to, never cleared: the caller clears them once and sums row blocks on
 *     the device, as with skf_complete_digits.  Integer atomics only: the counts do not depend on col_splits (0 = the library
 *     chooses, at most 32), the launch geometry or the order of arrival.
 *   P6: for every t, the sum of hist[b] over b > t (the increments of one call) equals *n_found of skf_complete_above on the
 *     same inputs with thr[r] = edges[t] in every row -- for every col_splits of either operator and every cut of the rows
 *     into blocks.
 *   P7: a counted target e lands in bin #{ t : edges[t] <= v }, v = out_val[e] of skf_complete_ranks on the same inputs: both
 *     scores are formed by the same chain of matrix instructions.
 *   Refused with SKF_E_INVALID before any HIP call: the operand checks of skf_complete_topk, n_edges outside 1 ..
 *     SKF_HIST_MAX_EDGES, edges or hist NULL, tgt_indptr / tgt_indices / hist_tgt not all NULL or all given (and n_targets != 0
 *     without them, n_targets < 0), col_splits outside 0 .. 32; SKF_E_WORKSPACE for a workspace that is NULL, too small or not
 *     256-byte aligned (skf_complete_hist_workspace_bytes: flag words only).  Refused with SKF_E_INVALID on the device, in one
 *     round trip, before anything is counted: exclusion or target lists that are not canonical (tgt_indptr[m] != n_targets
 *     included), a NaN edge, an edge smaller than the one before it.  Every refusal leaves both histograms, and the memory
 *     behind them, as they were.  m == 0 or n_cols == 0 succeeds and adds nothing.
 *   LDS: the edges and the bins are sized by n_edges and by whether targets are given; 16 edges do not pay for 2047.
 *   dtype SKF_F64 / SKF_F32 (the type of H, Gc and edges); 1 <= c <= 1024; m and n_cols < 2^31. */
#define SKF_HIST_MAX_EDGES 2047
int skf_complete_hist_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int64_t n_targets, int32_t col_splits,
                                      size_t* bytes);
int skf_complete_hist(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols,
                      int32_t c, const void* edges /* dtype [n_edges], device */, int32_t n_edges,
                      const int64_t* excl_indptr, const int32_t* excl_indices,
                      const int64_t* tgt_indptr, const int32_t* tgt_indices, int64_t n_targets,
                      uint64_t* hist /* device [n_edges + 1], ADDED to */,
                      uint64_t* hist_tgt /* device [n_edges + 1], ADDED to; NULL iff no targets */,
                      int32_t col_splits /* 0 = choose */, void* workspace, size_t workspace_bytes, void* stream);

/* The k-th best score of EVERY row of X = H Gc^T (H, Gc as for skf_complete_topk) for any k, without X: Recall@100 / @1000,
 * R-precision and candidate generation need per-row lists far beyond SKF_TOPK_MAX, and a row's k best columns are
 * skf_complete_above at the row's own k-th score.  One radix select per row over the keys of skf_complete_digits, in digits of
 * 7 bits (5 passes for SKF_F32, 10 for SKF_F64): a counting pass over the score tiles fills one histogram per row, one wave
 * per row extends the row's prefix, and so on -- every pass of one call is enqueued on the stream, nothing travels to the
 * host in between, and out_thr is a device array that skf_complete_above takes as it is.
 *   Candidates, scores and keys: as for skf_complete_digits, per row.  want (device, int64 [m], each >= 0): how many of row
 *     r's candidates are wanted.  With cands_r candidates in row r and n_r = min(want[r], cands_r):
 *       n_r == 0: out_thr[r] = NaN, out_greater[r] = out_equal[r] = 0;
 *       otherwise: out_thr[r] (dtype) = the n_r-th largest candidate score of the row, out_greater[r] = the candidates above it,
 *         out_equal[r] = the candidates equal to it: out_greater[r] < n_r <= out_greater[r] + out_equal[r].
 *     out_cands[r] = cands_r unless out_cands is NULL.  All outputs on the device.  Integer counts and integer atomics only: the
 *     outputs do not depend on col_splits (0 = the library chooses, at most 32), the launch geometry or the order of arrival.
 *   P4: skf_complete_above on the same inputs with thr = out_thr returns exactly out_greater[r] + out_equal[r] entries in row r,
 *     out_greater[r] of them above out_thr[r] -- for every col_splits of either operator and every cut of the rows into blocks.
 *     A NaN threshold selects nothing.
 *   P5: with want[r] = k <= SKF_TOPK_MAX, row r's P4 entries ordered by (value descending, column ascending) begin with
 *     skf_complete_topk's list for that k -- its first min(k, cands_r) slots -- index for index and bit for bit.
 *   Refused with SKF_E_INVALID: a NULL want, out_thr, out_greater or out_equal, the operand checks of skf_complete_topk,
 *     col_splits outside 0 .. 32, exclusion lists that are not canonical and a negative want[r] (both found on the device, in
 *     one round trip, before anything is counted); SKF_E_WORKSPACE for a workspace that is NULL, too small or not 256-byte
 *     aligned.  Every refusal leaves every output as it was; the argument checks answer before any HIP call.  The only host
 *     synchronisation is that of the list check.  m == 0 succeeds and writes nothing; n_cols == 0 succeeds without a product
 *     launch: every row gets NaN / 0.
 *   Workspace (skf_complete_row_kth_workspace_bytes): flag words, the row histograms (uint32 [m][128]) and two 64-bit words
 *     per row -- 528 m bytes and a little; it grows with m and never with m x n_cols.  skf_complete_topk keeps its limit.
 *   dtype SKF_F64 / SKF_F32 (the type of H, Gc and out_thr); 1 <= c <= 1024; m and n_cols < 2^31. */
int skf_complete_row_kth_workspace_bytes(int32_t dtype, int64_t m, int64_t n_cols, int32_t col_splits, size_t* bytes);
int skf_complete_row_kth(int32_t dtype, const void* H, int64_t ldh, int64_t m, const void* Gc, int64_t ldg, int64_t n_cols,
                         int32_t c, const int64_t* want /* device [m], each >= 0 */,
                         const int64_t* excl_indptr, const int32_t* excl_indices,
                         void* out_thr /* dtype [m], device */, int64_t* out_greater /* [m] */, int64_t* out_equal /* [m] */,
                         int64_t* out_cands /* [m] or NULL */, int32_t col_splits /* 0 = choose */,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- the column-mean initialisers on the device (reference _init.py:20-61: `random_c` :20-41, `random_vcol` :44-61) ----
 * The reference fills factor column k of an object type with the mean of take = int(0.2 m) randomly chosen columns of every
 * relation that touches the type, oriented so that the type's objects are its rows (V, n x m), and `random_c` draws them
 * from the half of the columns with the largest 2-norm: G = 1e-5 + sum over the views of |mean of the chosen columns|.
 * With W (m x c) the 0/1 matrix of the chosen columns the means are (V W) / take -- the contraction the plan runs for that
 * relation in every stored form (P = R G_j / Q = R^T G_i), with a right operand that is exact in bf16.  The random stream
 * stays on the host: the caller draws the indices and hands them over.
 *
 * Both operators take relations of a bound SKF_DFMF / SKF_DFMC plan that the plan holds WHOLE and UNMASKED: dense (the
 * engine's type; SKF_BF16: its padded bf16 copy or the bitmap of a SKF_REL_BINARY relation) or SKF_REL_SPARSE_CSR without
 * SKF_REL_FILL_RANK1.  SKF_E_INVALID, with a message, before any HIP call and with nothing written: a masked relation, one
 * given as its known entries, a rank-one fill, SKF_OPT_OWNED_ROWS plans and row blocks, SKF_TRANSFORM plans.  (A 0/1 relation
 * that SKF_BF16 keeps as lists of its ones beside its bitmap is read through the bitmap.)  The plan's own workspace is not touched: scratch is the caller's (256-byte aligned; NULL,
 * short or misaligned: SKF_E_WORKSPACE).
 *
 * skf_plan_relation_norms: the f64 sum of SQUARES of every row (row_sq[n_i]) and of every column (col_sq[n_j]) of relation
 * `rel` as stored -- device outputs, a null pointer is skipped; the caller takes the square roots.  One pass over a dense /
 * bitmap relation: partial sums over fixed slabs of rows and blocks of columns, stored and added first to last -- no atomics,
 * a grid fixed by the shape alone, the same bits on every run; a relation kept as lists: each line's stored entries in list
 * order (needs no scratch). */
int skf_plan_relation_norms_workspace_bytes(const skf_plan* plan, int32_t rel, size_t* bytes);
int skf_plan_relation_norms(skf_plan* plan, int32_t rel, double* row_sq, double* col_sq, void* workspace, size_t workspace_bytes,
                            void* stream);

/* One oriented view of skf_plan_init_column_means: relation `rel`, read as V = R when `type` is its row type and as V = R^T
 * when it is its column type; sel[c * take] (device, int32, row-major): row k holds the columns of V averaged into factor
 * column k.  The indices of one row are DISTINCT -- the caller's duty (an index given twice would count once, where the
 * reference's mean counts it twice); an index outside [0, m) is found on the device before anything is written:
 * SKF_E_INVALID.  take < 1 (a view of fewer than 5 columns, where the reference's mean of nothing is NaN) or take > m:
 * SKF_E_INVALID.  The size query reads rel and take only. */
typedef struct {
    int32_t rel;
    int32_t take;
    const int32_t* sel;
} skf_init_view;

/* G0 (n x c of `type`, device, MASTER type, leading dimension ld >= c; nothing past column c of a row is touched)
 *   = round( 1e-5 + sum over the views, in the order given, of | (V W) / (double)take | )
 * accumulated in f64 and rounded once.  The products run through the plan's contraction launches with W as the right operand
 * (bf16 operands and f32 accumulation for SKF_BF16, the master type otherwise), so data whose partial sums are exact --
 * 0/1 entries, small integers -- give the bits of the reference's float64 statement cast to the master type, in every engine.
 * The caller then hands G0 to skf_set_factor.  Scratch grows with m * c + n * c, never with n * m. */
int skf_plan_init_column_means_workspace_bytes(const skf_plan* plan, int32_t type, int32_t n_views, const skf_init_view* views,
                                               size_t* bytes);
int skf_plan_init_column_means(skf_plan* plan, int32_t type, int32_t n_views, const skf_init_view* views, void* G0, int64_t ld,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ... and for relations with MISSING values.  The four functions above refuse a relation whose unstored entries are not zero;
 * these take every form those take -- through the same launches, with the same bits -- and two more:
 *   known entries   the lists of a masked relation of a SKF_DFMC plan, built from its mask (known_bound) or handed over as
 *                   SKF_REL_KNOWN_CSR.  What lies beneath the unknown entries is the caller's constant: `fill` / fills[v].
 *   rank one        SKF_REL_SPARSE_CSR | SKF_REL_FILL_RANK1: an entry not stored holds a_r b_c, the lists hold d = v - a_r b_c.
 * With V (n x m) the oriented view, C_k the `take` columns of row k of sel, stored(r) the stored columns of line r in list order
 * (a, b in the view's orientation), everything in f64, every sum in list order, one owner per output element, no atomics:
 *   known entries   mean_rk = (sum over stored(r) in C_k of v_rc + (take - |stored(r) in C_k|) f) / take
 *                   sq_c    = sum over the stored rows of v_rc^2 + (n - cnt_c) f^2
 *   rank one        mean_rk = (sum over stored(r) in C_k of d_rc + a_r B_k) / take,  B_k = sum over C_k of b_c in the order of sel
 *                   sq_c    = sum over the stored rows of (d_rc + a_r b_c)^2 + b_c^2 (|a|^2 - sum over the stored rows of a_r^2)
 *   G0 = round(1e-5 + sum over the views, in the order given, of |mean|), the views over a fill and the products of the
 * other forms adding into one f64 accumulator.  The epilogues are a product, rounded, then a sum, rounded (no fused
 * multiply-add).  A view over a fill is one pass over its lists against m * c one-byte flags of the chosen columns -- a wave
 * per line, a long line serially in its wave -- so scratch grows with m * c bytes + n * c * 8, never with n * m.
 * Refused as above (SKF_E_INVALID, nothing written, no HIP call): a masked relation the plan keeps DENSE, SKF_OPT_OWNED_ROWS
 * plans, row blocks and absent relations, SKF_TRANSFORM plans and fold-in lists, and a fill that is not finite (read for
 * known-entry relations only; fills: host, one per view, may be NULL when no view is a known-entry relation).  Order of the
 * checks, the flag word, ld, alignment and SKF_E_WORKSPACE: as above.  The norms of the two list forms need no scratch. */
int skf_plan_relation_norms_filled_workspace_bytes(const skf_plan* plan, int32_t rel, size_t* bytes);
int skf_plan_relation_norms_filled(skf_plan* plan, int32_t rel, double fill, double* row_sq, double* col_sq, void* workspace,
                                   size_t workspace_bytes, void* stream);
int skf_plan_init_column_means_filled_workspace_bytes(const skf_plan* plan, int32_t type, int32_t n_views, const skf_init_view* views,
                                                      size_t* bytes);
int skf_plan_init_column_means_filled(skf_plan* plan, int32_t type, int32_t n_views, const skf_init_view* views,
                                      const double* fills /* host, [n_views]; read for known-entry views only */, void* G0, int64_t ld,
                                      void* workspace, size_t workspace_bytes, void* stream);

/* K = pinv(A) for symmetric A (n x n): f64 Jacobi eigen-decomposition + the singular-value
 * cut-off of scipy.linalg.pinv (reference _dfmf.py:232, _dfmc.py:307). */
int skf_pinv_sym_workspace_bytes(int32_t n, size_t* bytes);
int skf_pinv_sym(int32_t dtype, const void* A, int64_t lda, void* K, int64_t ldk, int32_t n,
                 void* workspace, size_t workspace_bytes, void* stream);

/* dst(r,c) = hash_uniform(seed, r*cols + c) * scale + shift  (synthetic benchmark data) */
int skf_fill_uniform(int32_t dtype, void* dst, int64_t rows, int64_t cols, int64_t ld,
                     uint64_t seed, double scale, double shift, void* stream);

/* Relation.filled() on the device (reference fusion_graph.py:464-510): every UNKNOWN entry of `data` (rows x cols,
 * SKF_F64 / SKF_F32, in place) -- not finite, or flagged in the optional byte mask -- is replaced by the mean of the
 * known entries of the whole matrix (strategy 0, 'mean'), of its row (1, 'row_mean') or column (2, 'col_mean'; rows /
 * columns without a known entry take the overall mean), or by `value` (3, a constant).  numpy.nanmean semantics: NaN
 * and masked entries are skipped, +-inf take part in the means.  Whether the mask survives the fill is the host
 * layer's business (it does for 'mean' and constants, not for the row / column means: fusion_graph.py:475-489). */
int skf_fill_unknown_workspace_bytes(int64_t rows, int64_t cols, size_t* bytes);
int skf_fill_unknown(int32_t dtype, void* data, int64_t ld, int64_t rows, int64_t cols, const uint8_t* mask,
                     int64_t mask_ld, int32_t strategy, double value, void* workspace, size_t workspace_bytes,
                     void* stream);

/* dst(r,c) = (dst_dtype) src(r,c), dtypes SKF_F64 / SKF_F32; SKF_E_INVALID for ldd < cols or lds < cols */
int skf_cast(int32_t dst_dtype, void* dst, int64_t ldd, int32_t src_dtype, const void* src,
             int64_t lds, int64_t rows, int64_t cols, void* stream);

/* Rows [*begin, *begin + *count) of a type of `n_obj` objects that process `part_index` of `part_count` owns under
 * SKF_OPT_OWNED_ROWS; *chunk = rows per process of the padded layout the exchanges use (equal for all processes, a multiple
 * of 256 for large types / of 64 for SKF_BF16; part_count * chunk >= n_obj, the last owners may hold fewer rows or none). */
int skf_owned_rows(int32_t dtype, int64_t n_obj, int32_t part_index, int32_t part_count, int64_t* begin, int64_t* count,
                   int64_t* chunk);

/* Kernel launches the calling thread has issued through this library so far (every plan, every entry point; a hipGraph
 * replay counts the launches it was captured from once, at capture).  Callers take differences: launches per iteration of a
 * schedule are part of its latency budget (bench.py reports them for the rank-of-8 emulation). */
int skf_launch_count(int64_t* launches);

/* Split-K launches of the calling thread whose slice count was CLAMPED because the scratch sized at plan creation could not
 * hold the slices the launch-time model asked for (run_gemm: safe, but the modelled schedule is then not the executed one;
 * advisor, round 5).  Zero for every plan the tests and the benchmark create; a non-zero count names a sizing rule
 * (skf_plan_create: want_part) that has fallen behind the tile / slice pickers.  The stand-alone products (skf_gemm*)
 * run on the caller's scratch and are not counted. */
int skf_split_clamps(int64_t* clamps);

/* Held-out pairs scored inside the fit: early stopping on data the model never trained on, and the best iterate kept.  The
 * reference's `stopping` / `stopping_system` (_dfmf.py:212-221, 301-322) read the training objective, which keeps falling
 * while the model overfits.  A MONITORED plan scores lists of held-out (row, column, value) triples after every iteration
 * of skf_iterate, on the same stream, judges the result on the device and keeps a device copy of the best (G, S); the host
 * reads the verdict when it likes (skf_plan_get_monitor) and is never needed to decide.
 *   A list: COO of one relation, rows (int32, NON-DECREASING), cols (int32, any order), values (the plan's master type:
 *     double for SKF_F64, float for SKF_F32 / SKF_BF16), n >= 1 entries; duplicate pairs are allowed.  Device pointers, owned
 *     by the caller, valid while attached.  At most one list per relation.
 *   Squared error of list l under (G, S): sum over its entries of ((double)v - (double)x)^2, x = <(G_i S)[row], G_j[col]> with
 *     exactly the bits skf_complete_entries returns on the same H = G_i S and G_j (16 lanes per entry, fixed fold).  A slab
 *     of 1024 entries is one workgroup and one f64 partial, added in a fixed order; a list's total is its partials first to
 *     last.  No atomics: two runs give the same bits, and the grid depends on n alone.  H is formed in the master type (the
 *     SKF_BF16 engine scores on its f32 masters) by the product the plan's own H = G_i S goes through, on scratch of the
 *     monitor's workspace.
 *   Judge (one workgroup, after every iteration): history[it * n_lists + l] = the error of list l while it < capacity_iters;
 *     total = the errors added in list order (the POOLED criterion).  The first total that is not NaN is an improvement;
 *     afterwards total < best - min_delta is; a NaN total never improves.  An improvement records best, best_iter (1-based:
 *     the number of iterations of the best model) and lets the snapshot -- every factor master and every backbone -- be
 *     taken; anything else counts one more iteration without improvement, and with patience > 0, patience such iterations
 *     in a row stop the monitor: best, best_iter and the snapshot are frozen from then on (stop_iter: the iteration that
 *     stopped it).  Iterations issued after that still run and are still scored into the history; the plan's own state is
 *     never rewritten.
 *   skf_plan_heldout_workspace_bytes: bytes of the monitor's workspace -- 256 B of state words, the slab partials, per list H
 *     (n_i x c_j) and its split-K scratch, the history (capacity_iters * n_lists * 8 B) and one snapshot of all factors and
 *     backbones; nothing of size n_i x n_j.
 *   skf_plan_set_heldout: on a bound SKF_DFMF / SKF_DFMC plan without row blocks, owned rows or a communicator; the rank of
 *     a list's column type at most 1024; the workspace 256-byte aligned and at least that large.  The lists are validated on
 *     the device before anything gathers through them (indices in range, rows non-decreasing, values finite).  Every
 *     refusal is SKF_E_INVALID (SKF_E_STATE: not bound) and leaves the plan UNMONITORED; n_lists = 0 detaches.  Binding a
 *     workspace again detaches too.  A monitored plan never replays a hipGraph and does not batch (skf_plan_batchable: 0).
 *   skf_plan_heldout_sqerr: out_dev[l] (device, n_lists f64) = the squared error of list l under the current (G, S) -- what
 *     skf_get_factor / skf_get_backbone return now, the convention of skf_relation_sqerr.  Judges nothing.
 *   skf_plan_get_heldout_product: H of list `list` as the last evaluation left it (verification accessor), master type.
 *   skf_plan_get_monitor: synchronises; any output pointer may be NULL.  history_host (HOST memory, `capacity` rows of n_lists
 *     f64) receives min(seen, capacity_iters, capacity) rows.
 *   skf_get_best_factor / skf_get_best_backbone: as skf_get_factor / skf_get_backbone, out of the snapshot; SKF_E_STATE
 *     while no judged iteration has improved. */
typedef struct skf_heldout_desc {
    int32_t rel;
    int64_t n;
    const int32_t* rows;
    const int32_t* cols;
    const void* values;
} skf_heldout_desc;
int skf_plan_heldout_workspace_bytes(const skf_plan* plan, int32_t n_lists, const skf_heldout_desc* descs, int64_t capacity_iters,
                                     size_t* bytes);
int skf_plan_set_heldout(skf_plan* plan, int32_t n_lists, const skf_heldout_desc* descs, int32_t patience, double min_delta,
                         int64_t capacity_iters, void* workspace, size_t workspace_bytes, void* stream);
int skf_plan_heldout_sqerr(skf_plan* plan, double* out_dev, void* stream);
int skf_plan_get_heldout_product(const skf_plan* plan, int32_t list, void* H, int64_t ld, void* stream);
int skf_plan_get_monitor(const skf_plan* plan, int64_t* seen, int64_t* best_iter, int64_t* stop_iter, int32_t* stopped, double* best,
                         double* history_host, int64_t capacity, void* stream);
int skf_get_best_factor(const skf_plan* plan, int32_t type, void* G, int64_t ld, void* stream);
int skf_get_best_backbone(const skf_plan* plan, int32_t rel, void* S, int64_t ld, void* stream);

const char* skf_last_error(void);
const char* skf_version(void);
/* Layout version of the structs and signatures above (SKF_ABI_VERSION).  A binding built against another version must not
 * call the library: descriptors grew between versions (skf_relation_desc.known_bound: 3, skf_options.flags: 4; version 5
 * adds entry points only -- skf_small_graph_limits, skf_comm_info, skf_launch_count; later: skf_fold_lists and the flag
 * SKF_REL_FOLD_CSR; skf_fold_known_pass and the flag SKF_REL_FOLD_KNOWN; skf_complete_topk_workspace_bytes, skf_complete_topk, skf_complete_entries and SKF_TOPK_MAX;
 * skf_get_constraint_lists and the flag SKF_OPT_THETA_OWNED_ROWS; skf_plan_set_relation_fill and the flag SKF_REL_FILL_RANK1;
 * skf_complete_ranks_workspace_bytes and skf_complete_ranks; skf_complete_above_workspace_bytes and skf_complete_above;
 * skf_plan_relation_norms, skf_plan_init_column_means, their workspace queries and skf_init_view, a struct of their own -- the
 * structs before it are those of version 4; skf_complete_digits_workspace_bytes and skf_complete_digits;
 * skf_complete_row_kth_workspace_bytes and skf_complete_row_kth; skf_plan_relation_norms_filled,
 * skf_plan_init_column_means_filled and their workspace queries; skf_complete_hist_workspace_bytes, skf_complete_hist and
 * SKF_HIST_MAX_EDGES; skf_heldout_desc, a struct of its own, skf_plan_heldout_workspace_bytes, skf_plan_set_heldout,
 * skf_plan_heldout_sqerr, skf_plan_get_heldout_product, skf_plan_get_monitor, skf_get_best_factor and skf_get_best_backbone). */
#define SKF_ABI_VERSION 5
int skf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SKFUSION_HIP_H */
