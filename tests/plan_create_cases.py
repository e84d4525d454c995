"""Every refusal of skf_plan_create, by status and FULL text of skf_last_error(), and which refusal answers where one
descriptor earns two.  The texts are written from the SKF_FAIL lines of plan creation (in csrc/skf_api.hip when this table
was written, since then in csrc/skf_create.inc; the entry point's own stay in csrc/skf_api.hip) and from
include/skfusion_hip.h, the order from the order of those lines -- not taken from a run.  No
HIP call is made before the validation answers, so nothing here launches a kernel: the same table runs on the host
emulator (tests/test_plan_create_emul.py) and against the product library (tests/test_gpu_plan_create.py).

Two types of 40 and 30 objects, ranks 4 and 3 (a third of 20 / 8 where a case needs one); SKF_BF16 row blocks: 128 / 64.

Three refusals cannot be reached through the entry point and have no case: the rank halves of the three "beyond the list
limits" texts (a rank above 1023 is refused with its object type), and "SKF_REL_FOLD_CSR excludes SKF_REL_KNOWN_CSR /
SKF_REL_SPARSE_CSR" as a whole -- on a fold-in plan either CSR flag is refused for the plan's variant first, on any other
plan the fold-in flag is (the four `fold + ...` pairs below pin exactly that)."""
import ctypes as C

import skfusion_amd._native as nat
from helpers import plan_create_status

BAD = nat.SKF_E_INVALID
F64, F32, BF16 = nat.SKF_F64, nat.SKF_F32, nat.SKF_BF16
DFMF, DFMC, TRANSFORM = nat.SKF_DFMF, nat.SKF_DFMC, nat.SKF_TRANSFORM
MFMA, VALU = nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU
ABSENT, NO_COL, MASKED, BITS, BINARY = (nat.SKF_REL_ABSENT, nat.SKF_REL_NO_COL_SIDE, nat.SKF_REL_MASKED,
                                        nat.SKF_REL_MASK_BITS, nat.SKF_REL_BINARY)
LISTS, KNOWN, SPARSE, FOLD, RANK1, FOLD_KNOWN = (nat.SKF_REL_KNOWN_LISTS, nat.SKF_REL_KNOWN_CSR, nat.SKF_REL_SPARSE_CSR,
                                                 nat.SKF_REL_FOLD_CSR, nat.SKF_REL_FILL_RANK1, nat.SKF_REL_FOLD_KNOWN)
OWNED, THETA_OWNED = nat.SKF_OPT_OWNED_ROWS, nat.SKF_OPT_THETA_OWNED_ROWS

_KEEP = C.create_string_buffer(64)
PTR = C.addressof(_KEEP)                    # a non-null `data` / `mask`: plan creation looks at the pointer, never through it

TWO = [(40, 4), (30, 3)]
THREE = TWO + [(20, 8)]
TWO64 = [(128, 4), (64, 3)]
OVER = 2000000001                           # one entry more than the lists take


def rel(flags=0, row=0, col=1, data=False, ld=None, mask=False, mask_ld=0, begin=0, rows=0, known=0, cols=30):
    """One relation descriptor.  A relation without a CSR / fold-in flag is dense: it gets its data pointer and ld = `cols`
    unless told otherwise (data=None: no pointer)."""
    dense = not (flags & (KNOWN | SPARSE | FOLD | ABSENT))
    d = dict(row_type=row, col_type=col, flags=flags, row_begin=begin, n_rows=rows, known_bound=known, mask_ld=mask_ld)
    if data or (dense and data is not None):
        d['data'] = PTR
    d['ld'] = ld if ld is not None else (cols if 'data' in d else 0)
    if mask:
        d['mask'] = PTR
    return d


def theta(type=0, data=True, ld=40, nnz=0):
    return dict(type=type, data=PTR if data else None, ld=ld if data else 0, nnz=nnz)


R = 'relation 0: '
FILL_TEXT = (R + 'SKF_REL_FILL_RANK1 goes with SKF_REL_SPARSE_CSR on SKF_DFMF / SKF_DFMC plans of whole relations '
             '(no SKF_OPT_OWNED_ROWS, no fold-in)')
WHOLE_TEXT = (R + 'SKF_REL_KNOWN_CSR / SKF_REL_SPARSE_CSR relations are whole relations (or the owned rows of a '
              'SKF_OPT_OWNED_ROWS plan)')
OWNED_TEXT = R + 'SKF_OPT_OWNED_ROWS wants the rows [%d, +%d) of its row type here (skf_owned_rows)'
ENTRIES_TEXT = ('constraint 0: a constraint given as its entries is for plans of whole relations (no row blocks, slices or '
                'SKF_OPT_OWNED_ROWS)')

# id -> (expected text, keyword arguments of helpers.plan_create_status after `lib`).  Python keeps the order written.
REFUSALS = {}


def case(name, text, types, relations=(), thetas=(), **options):
    assert name not in REFUSALS, name
    REFUSALS[name] = (text, dict(types=types, relations=list(relations), thetas=list(thetas), **options))


# ---- the entry point's own checks (skf_api.hip) ---------------------------------------------------------------------------
case('entry-no-types', 'null argument / no object types', [])
case('entry-dtype', 'unknown dtype 7', TWO, [rel()], dtype=7)
case('entry-bf16-valu', 'SKF_BF16 needs the MFMA engine', TWO, [rel()], dtype=BF16, engine=VALU)
case('entry-variant', 'bad variant', TWO, [rel()], variant=3)
case('entry-variant-negative', 'bad variant', TWO, [rel()], variant=-1)
case('entry-engine', 'bad engine', TWO, [rel()], engine=2)
case('pair-dtype-before-variant', 'unknown dtype 7', TWO, [rel()], dtype=7, variant=3)
case('pair-bf16-valu-before-variant', 'SKF_BF16 needs the MFMA engine', TWO, [rel()], dtype=BF16, engine=VALU, variant=3)
case('pair-variant-before-engine', 'bad variant', TWO, [rel()], variant=3, engine=2)

# ---- options and object types ---------------------------------------------------------------------------------------------
case('target-beyond', 'target type 2 out of range', TWO, [rel(cols=30)], variant=TRANSFORM, target=2)
case('target-none', 'target type -1 out of range', TWO, [rel()], variant=TRANSFORM, target=-1)
case('type-no-objects', 'object type 0: n_obj=0 rank=4 invalid', [(0, 4), (30, 3)], [rel()])
case('type-rank-zero', 'object type 1: n_obj=30 rank=0 invalid', [(40, 4), (30, 0)], [rel()])
case('type-rank-1024', 'object type 1: n_obj=30 rank=1024 invalid', [(40, 4), (30, 1024)], [rel()])
case('type-too-large', 'object type 0 too large', [(OVER, 4), (30, 3)], [rel()])
case('owned-part-index', 'SKF_OPT_OWNED_ROWS: part_index 2 outside [0, 2)', TWO, [rel()], part=(2, 2), opt_flags=OWNED)
case('owned-no-parts', 'SKF_OPT_OWNED_ROWS: part_index 0 outside [0, 0)', TWO, [rel()], part=(0, 0), opt_flags=OWNED)
case('sliced-part-index', 'part_index 3 outside [0, 2)', TWO, [rel()], part=(3, 2))
case('sliced-part-negative', 'part_index -1 outside [0, 2)', TWO, [rel()], part=(-1, 2))
case('theta-owned-alone', 'SKF_OPT_THETA_OWNED_ROWS needs SKF_OPT_OWNED_ROWS', TWO, [rel()], opt_flags=THETA_OWNED)
case('owned-transform', 'SKF_OPT_OWNED_ROWS is for SKF_DFMF / SKF_DFMC plans', TWO, [rel(FOLD, known=10)], variant=TRANSFORM,
     target=0, part=(0, 2), opt_flags=OWNED)
case('pair-target-before-type', 'target type 2 out of range', [(0, 4), (30, 3)], [rel()], variant=TRANSFORM, target=2)
case('pair-type-before-part-index', 'object type 0: n_obj=0 rank=4 invalid', [(0, 4), (30, 3)], [rel()], part=(2, 2), opt_flags=OWNED)
case('pair-part-index-before-later-type', 'part_index 3 outside [0, 2)', [(40, 4), (30, 0)], [rel()], part=(3, 2))
case('pair-part-index-before-theta-owned', 'part_index 3 outside [0, 2)', TWO, [rel()], part=(3, 2), opt_flags=THETA_OWNED)
case('pair-types-before-relations', 'SKF_OPT_THETA_OWNED_ROWS needs SKF_OPT_OWNED_ROWS', TWO, [rel(row=1, col=1)], opt_flags=THETA_OWNED)
case('pair-owned-transform-before-relations', 'SKF_OPT_OWNED_ROWS is for SKF_DFMF / SKF_DFMC plans', TWO, [rel(SPARSE, known=10)],
     variant=TRANSFORM, target=0, part=(0, 2), opt_flags=OWNED)

# ---- one relation: which flags go together, and with which plan ---------------------------------------------------------------
case('rel-type-index', R + 'type index out of range', TWO, [rel(row=2)])
case('rel-type-index-negative', R + 'type index out of range', TWO, [rel(col=-1)])
case('rel-same-type', R + 'row type == column type (pass it as a constraint)', TWO, [rel(row=1, col=1)])
case('known-csr-dfmf', R + 'SKF_REL_KNOWN_CSR needs SKF_DFMC', TWO, [rel(KNOWN, known=10)])
case('known-csr-transform', R + 'SKF_REL_KNOWN_CSR needs SKF_DFMC', TWO, [rel(KNOWN, known=10)], variant=TRANSFORM, target=0)
case('known-csr-data', R + 'SKF_REL_KNOWN_CSR takes no data / mask', TWO, [rel(KNOWN, known=10, data=True)], variant=DFMC)
case('known-csr-mask', R + 'SKF_REL_KNOWN_CSR takes no data / mask', TWO, [rel(KNOWN, known=10, mask=True, mask_ld=30)], variant=DFMC)
case('known-and-sparse', R + 'SKF_REL_KNOWN_CSR and SKF_REL_SPARSE_CSR exclude each other', TWO, [rel(KNOWN | SPARSE, known=10)],
     variant=DFMC)
case('sparse-transform', R + 'SKF_REL_SPARSE_CSR is for SKF_DFMF / SKF_DFMC plans', TWO, [rel(SPARSE, known=10)], variant=TRANSFORM,
     target=0)
case('sparse-data', R + 'SKF_REL_SPARSE_CSR takes no data / mask', TWO, [rel(SPARSE, known=10, data=True)])
case('sparse-mask', R + 'SKF_REL_SPARSE_CSR takes no data / mask', TWO, [rel(SPARSE, known=10, mask=True, mask_ld=30)], variant=DFMC)
case('sparse-masked-flag', R + 'SKF_REL_SPARSE_CSR takes no data / mask', TWO, [rel(SPARSE | MASKED, known=10)], variant=DFMC)
case('sparse-mask-bits-flag', R + 'SKF_REL_SPARSE_CSR takes no data / mask', TWO, [rel(SPARSE | BITS, known=10)])
case('fold-dfmf', R + 'SKF_REL_FOLD_CSR is for SKF_TRANSFORM plans', TWO, [rel(FOLD, known=10)])
case('fold-dfmc', R + 'SKF_REL_FOLD_CSR is for SKF_TRANSFORM plans', TWO, [rel(FOLD, known=10)], variant=DFMC)
case('fold-known-dfmf', R + 'SKF_REL_FOLD_KNOWN is for SKF_TRANSFORM plans', TWO, [rel(FOLD_KNOWN)])
case('fold-known-alone', R + 'SKF_REL_FOLD_KNOWN goes with SKF_REL_FOLD_CSR', TWO, [rel(FOLD_KNOWN)], variant=TRANSFORM, target=0)
case('fill-alone', FILL_TEXT, TWO, [rel(RANK1)])
case('fill-known-csr', FILL_TEXT, TWO, [rel(RANK1 | KNOWN, known=10)], variant=DFMC)
case('fill-absent', FILL_TEXT, TWO, [rel(RANK1 | SPARSE | ABSENT)], part=(0, 2))
case('fill-owned', FILL_TEXT, TWO, [rel(RANK1 | SPARSE, known=10, rows=20)], part=(0, 2), opt_flags=OWNED)
case('fill-fold', FILL_TEXT, TWO, [rel(RANK1 | FOLD, known=10)], variant=TRANSFORM, target=0)
case('fold-data', R + 'SKF_REL_FOLD_CSR takes no data / mask', TWO, [rel(FOLD, known=10, data=True)], variant=TRANSFORM, target=0)
case('fold-masked-flag', R + 'SKF_REL_FOLD_CSR takes no data / mask', TWO, [rel(FOLD | MASKED, known=10)], variant=TRANSFORM, target=0)
case('dense-no-data', R + 'dimension mismatch (ld 30 < 30 columns)', TWO, [rel(data=None, ld=30)])
case('dense-ld', R + 'dimension mismatch (ld 29 < 30 columns)', TWO, [rel(ld=29)])
# pairs, in the order of the lines
case('pair-type-index-before-same-type', R + 'type index out of range', TWO, [rel(row=5, col=5)])
case('pair-known-and-sparse-on-dfmf', R + 'SKF_REL_KNOWN_CSR needs SKF_DFMC', TWO, [rel(KNOWN | SPARSE, known=10)])
case('pair-known-data-before-sparse', R + 'SKF_REL_KNOWN_CSR takes no data / mask', TWO, [rel(KNOWN | SPARSE, known=10, data=True)],
     variant=DFMC)
case('pair-sparse-transform-before-mask', R + 'SKF_REL_SPARSE_CSR is for SKF_DFMF / SKF_DFMC plans', TWO,
     [rel(SPARSE | MASKED, known=10)], variant=TRANSFORM, target=0)
case('pair-fold-known-csr-on-transform', R + 'SKF_REL_KNOWN_CSR needs SKF_DFMC', TWO, [rel(FOLD | KNOWN, known=10)], variant=TRANSFORM,
     target=0)
case('pair-fold-sparse-on-transform', R + 'SKF_REL_SPARSE_CSR is for SKF_DFMF / SKF_DFMC plans', TWO, [rel(FOLD | SPARSE, known=10)],
     variant=TRANSFORM, target=0)
case('pair-fold-known-csr-on-dfmc', R + 'SKF_REL_FOLD_CSR is for SKF_TRANSFORM plans', TWO, [rel(FOLD | KNOWN, known=10)], variant=DFMC)
case('pair-fold-sparse-on-dfmf', R + 'SKF_REL_FOLD_CSR is for SKF_TRANSFORM plans', TWO, [rel(FOLD | SPARSE, known=10)])
case('pair-fold-with-fold-known-on-dfmc', R + 'SKF_REL_FOLD_CSR is for SKF_TRANSFORM plans', TWO, [rel(FOLD | FOLD_KNOWN, known=10)],
     variant=DFMC)
case('pair-fold-known-alone-on-dfmc', R + 'SKF_REL_FOLD_KNOWN is for SKF_TRANSFORM plans', TWO, [rel(FOLD_KNOWN)], variant=DFMC)
case('pair-fold-data-on-dfmf', R + 'SKF_REL_FOLD_CSR is for SKF_TRANSFORM plans', TWO, [rel(FOLD, known=10, data=True)])
case('pair-fold-known-alone-before-fill', R + 'SKF_REL_FOLD_KNOWN goes with SKF_REL_FOLD_CSR', TWO, [rel(FOLD_KNOWN | RANK1)],
     variant=TRANSFORM, target=0)
case('pair-sparse-fill-on-transform', R + 'SKF_REL_SPARSE_CSR is for SKF_DFMF / SKF_DFMC plans', TWO, [rel(SPARSE | RANK1, known=10)],
     variant=TRANSFORM, target=0)
case('pair-fill-before-fold-data', FILL_TEXT, TWO, [rel(RANK1 | FOLD, known=10, data=True)], variant=TRANSFORM, target=0)
case('pair-fill-before-dimension', FILL_TEXT, TWO, [rel(RANK1, data=None)])
case('pair-fill-owned-row-block', FILL_TEXT, TWO, [rel(RANK1 | SPARSE, known=10, begin=4, rows=24)], part=(0, 2), opt_flags=OWNED)
case('pair-fill-before-row-block-range', FILL_TEXT, TWO, [rel(RANK1, begin=30, rows=20)])

# ---- one relation: its rows, its mask, the plan's target and ownership ----------------------------------------------------------
BLOCK = R + 'row block [%d, +%d) outside the 40 objects of its row type'
case('block-begin-negative', BLOCK % (-1, 0), TWO, [rel(begin=-1)])
case('block-rows-negative', BLOCK % (0, -1), TWO, [rel(rows=-1)])
case('block-beyond', BLOCK % (30, 20), TWO, [rel(begin=30, rows=20)], part=(0, 2))
case('sparse-block', WHOLE_TEXT, TWO, [rel(SPARSE, known=10, rows=20)])
case('known-csr-block', WHOLE_TEXT, TWO, [rel(KNOWN, known=10, begin=20, rows=20)], variant=DFMC, part=(1, 2))
case('sparse-absent', WHOLE_TEXT, TWO, [rel(SPARSE | ABSENT)], part=(0, 2))
case('sparse-no-col-side', WHOLE_TEXT, TWO, [rel(SPARSE | NO_COL, known=10)])
case('fold-block', R + 'SKF_REL_FOLD_CSR relations are whole relations', TWO, [rel(FOLD, known=10, rows=20)], variant=TRANSFORM, target=0)
case('fold-absent', R + 'SKF_REL_FOLD_CSR relations are whole relations', TWO, [rel(FOLD | ABSENT)], variant=TRANSFORM, target=0)
case('transform-block', R + 'row blocks are for SKF_DFMF / SKF_DFMC plans', TWO, [rel(rows=20)], variant=TRANSFORM, target=0)
case('bf16-block-begin', R + 'SKF_BF16 row blocks must start at a multiple of 64', TWO64, [rel(begin=32, rows=64, cols=64)], dtype=BF16,
     part=(0, 2))
case('mask-dfmf', R + 'masks need SKF_DFMC', TWO, [rel(mask=True, mask_ld=30)])
case('masked-flag-dfmf', R + 'masks need SKF_DFMC', TWO, [rel(MASKED)])
case('mask-transform', R + 'masks need SKF_DFMC', TWO, [rel(mask=True, mask_ld=30)], variant=TRANSFORM, target=0)
case('mask-ld-bytes', R + 'mask ld', TWO, [rel(mask=True, mask_ld=29)], variant=DFMC)
case('mask-ld-bits', R + 'mask ld', TWO, [rel(BITS, mask=True, mask_ld=3)], variant=DFMC)
case('transform-off-target', 'relation 0 must include the target object type', THREE, [rel()], variant=TRANSFORM, target=2)
case('owned-whole-relation', OWNED_TEXT % (0, 20), TWO, [rel()], part=(0, 2), opt_flags=OWNED)
case('owned-other-rank-rows', OWNED_TEXT % (20, 20), TWO, [rel(begin=0, rows=20)], part=(1, 2), opt_flags=OWNED)
case('owned-absent-with-rows', OWNED_TEXT % (0, 20), TWO, [rel(ABSENT)], part=(0, 2), opt_flags=OWNED)
# (SKF_BF16: chunks of 64 rows -- rank 1 of 2 owns rows 64 .. 127 of 128, and nothing of the 64 of the other type)
case('owned-bf16-chunk', OWNED_TEXT % (64, 64), TWO64, [rel(begin=64, rows=32, cols=64)], dtype=BF16, part=(1, 2), opt_flags=OWNED)
case('owned-not-absent-without-rows', OWNED_TEXT % (64, 0), TWO64, [rel(row=1, col=0, cols=128)], dtype=BF16, part=(1, 2), opt_flags=OWNED)
case('bound-negative', R + 'negative bound on the known entries', TWO, [rel(known=-1)])
case('bound-negative-second-relation', 'relation 1: negative bound on the known entries', TWO, [rel(), rel(SPARSE, known=-1)])
case('fold-too-many', R + 'SKF_REL_FOLD_CSR beyond the list limits (a rank above 1024 or 2000000001 > 2e9 entries)', TWO,
     [rel(FOLD, known=OVER)], variant=TRANSFORM, target=0)
# pairs, in the order of the lines
case('pair-dimension-before-row-block', R + 'dimension mismatch (ld 0 < 30 columns)', TWO, [rel(data=None, begin=30, rows=20)])
case('pair-row-block-range-before-whole', BLOCK % (30, 20), TWO, [rel(SPARSE, known=10, begin=30, rows=20)])
case('pair-whole-before-bf16-begin', WHOLE_TEXT, TWO64, [rel(SPARSE, known=10, begin=32, rows=64)], dtype=BF16)
case('pair-fold-block-on-transform', R + 'SKF_REL_FOLD_CSR relations are whole relations', TWO64, [rel(FOLD, known=10, begin=32, rows=64)],
     variant=TRANSFORM, target=0, dtype=BF16)
case('pair-transform-block-before-bf16-begin', R + 'row blocks are for SKF_DFMF / SKF_DFMC plans', TWO64,
     [rel(begin=32, rows=64, cols=64)], variant=TRANSFORM, target=0, dtype=BF16)
case('pair-transform-block-before-target', R + 'row blocks are for SKF_DFMF / SKF_DFMC plans', THREE, [rel(rows=20)], variant=TRANSFORM,
     target=2)
case('pair-bf16-begin-before-mask', R + 'SKF_BF16 row blocks must start at a multiple of 64', TWO64,
     [rel(begin=32, rows=64, cols=64, mask=True, mask_ld=64)], dtype=BF16)
case('pair-masks-need-dfmc-before-mask-ld', R + 'masks need SKF_DFMC', TWO, [rel(mask=True, mask_ld=29)])
case('pair-mask-before-target', R + 'masks need SKF_DFMC', THREE, [rel(MASKED)], variant=TRANSFORM, target=2)
case('pair-mask-ld-before-owned-rows', R + 'mask ld', TWO, [rel(mask=True, mask_ld=29)], variant=DFMC, part=(0, 2), opt_flags=OWNED)
case('pair-target-before-bound', 'relation 0 must include the target object type', THREE, [rel(known=-1)], variant=TRANSFORM, target=2)
case('pair-owned-rows-before-bound', OWNED_TEXT % (0, 20), TWO, [rel(known=-1)], part=(0, 2), opt_flags=OWNED)
case('pair-bound-sign-before-fold-limits', R + 'negative bound on the known entries', TWO, [rel(FOLD, known=-1)], variant=TRANSFORM,
     target=0)
case('pair-first-relation-answers', R + 'negative bound on the known entries', TWO, [rel(known=-1), rel(row=2)])

# ---- which relations are kept as lists -------------------------------------------------------------------------------------------
case('sparse-sliced', R + 'SKF_REL_SPARSE_CSR is for plans of whole relations or of owned rows', TWO, [rel(SPARSE, known=10)],
     part=(0, 2))
case('sparse-beside-a-block', 'relation 1: SKF_REL_SPARSE_CSR is for plans of whole relations or of owned rows', TWO,
     [rel(rows=20), rel(SPARSE, known=10)])
case('sparse-too-many', R + 'SKF_REL_SPARSE_CSR beyond the list limits (a rank above 1024 or 2000000001 > 2e9 entries)', TWO,
     [rel(SPARSE, known=OVER)])
case('known-csr-sliced', R + 'SKF_REL_KNOWN_CSR is for plans of whole relations or of owned rows', TWO, [rel(KNOWN, known=10)],
     variant=DFMC, part=(0, 2))
case('known-csr-too-many', R + 'SKF_REL_KNOWN_CSR beyond the list limits (rank 4 > 1024 or 2000000001 > 2e9 entries)', TWO,
     [rel(KNOWN, known=OVER)], variant=DFMC)
LISTS_TEXT = R + 'SKF_REL_KNOWN_LISTS needs a bound on the known entries of the local rows'
case('known-lists-no-bound', LISTS_TEXT, TWO, [rel(MASKED | LISTS, rows=20, mask=True, mask_ld=30)], variant=DFMC, part=(0, 2),
     opt_flags=OWNED)
case('known-lists-no-mask-here', LISTS_TEXT, TWO, [rel(MASKED | LISTS, rows=20, known=10)], variant=DFMC, part=(0, 2), opt_flags=OWNED)
case('known-lists-too-many', LISTS_TEXT, TWO, [rel(MASKED | LISTS, rows=20, mask=True, mask_ld=30, known=OVER)], variant=DFMC, part=(0, 2),
     opt_flags=OWNED)
case('pair-sliced-before-limits', R + 'SKF_REL_SPARSE_CSR is for plans of whole relations or of owned rows', TWO,
     [rel(SPARSE, known=OVER)], part=(0, 2))
case('pair-known-csr-sliced-before-limits', R + 'SKF_REL_KNOWN_CSR is for plans of whole relations or of owned rows', TWO,
     [rel(KNOWN, known=OVER)], variant=DFMC, part=(0, 2))
case('pair-every-description-before-any-list', 'relation 1: row type == column type (pass it as a constraint)', TWO,
     [rel(SPARSE, known=10), rel(row=1, col=1)], part=(0, 2))
case('pair-lists-before-constraints', R + 'SKF_REL_SPARSE_CSR is for plans of whole relations or of owned rows', TWO,
     [rel(SPARSE, known=10)], [theta(type=2)], part=(0, 2))

# ---- constraints -----------------------------------------------------------------------------------------------------------------
case('theta-type', 'constraint 0 invalid', TWO, [rel()], [theta(type=2)])
case('theta-type-negative', 'constraint 0 invalid', TWO, [rel()], [theta(type=-1)])
case('theta-ld', 'constraint 1 invalid', TWO, [rel()], [theta(), theta(ld=39)])
case('theta-off-target', 'constraint 0 must be on the target object type', TWO, [rel(FOLD, known=10)], [theta(type=1, ld=30)],
     variant=TRANSFORM, target=0)
case('theta-nnz-negative', 'constraint 0: negative non-zero bound', TWO, [rel()], [theta(nnz=-1)])
case('theta-entries-sliced', ENTRIES_TEXT, TWO, [rel()], [theta(data=False, nnz=10)], part=(0, 2))
case('theta-entries-beside-a-block', ENTRIES_TEXT, TWO, [rel(rows=20)], [theta(data=False, nnz=10)])
case('theta-entries-owned', ENTRIES_TEXT, TWO, [rel(rows=20)], [theta(data=False, nnz=10)], part=(0, 2), opt_flags=OWNED)
case('theta-entries-too-many', 'constraint 0: 2000000001 > 2e9 entries', TWO, [rel()], [theta(data=False, nnz=OVER)])
case('pair-theta-invalid-before-target', 'constraint 0 invalid', TWO, [rel(FOLD, known=10)], [theta(type=2)], variant=TRANSFORM, target=0)
case('pair-theta-target-before-nnz', 'constraint 0 must be on the target object type', TWO, [rel(FOLD, known=10)],
     [theta(type=1, ld=30, nnz=-1)], variant=TRANSFORM, target=0)
case('pair-theta-nnz-sign-before-entries', 'constraint 0: negative non-zero bound', TWO, [rel()], [theta(data=False, nnz=-1)], part=(0, 2))
case('pair-theta-sliced-before-too-many', ENTRIES_TEXT, TWO, [rel()], [theta(data=False, nnz=OVER)], part=(0, 2))
case('pair-first-constraint-answers', 'constraint 0: 2000000001 > 2e9 entries', TWO, [rel()], [theta(data=False, nnz=OVER), theta(type=2)])

# Descriptors the refusals above were cut from, accepted as they stand: the form, the plan, the block a case then breaks.
ACCEPTED = {
    'dense': dict(types=TWO, relations=[rel()]),
    'dense-valu-f32': dict(types=TWO, relations=[rel()], dtype=F32, engine=VALU),
    'rank-1023': dict(types=[(40, 4), (30, 1023)], relations=[rel()]),
    'masked-bytes': dict(types=TWO, relations=[rel(mask=True, mask_ld=30, known=10)], variant=DFMC),
    'masked-bits': dict(types=TWO, relations=[rel(BITS, mask=True, mask_ld=4, known=10)], variant=DFMC),
    'known-csr': dict(types=TWO, relations=[rel(KNOWN, known=10)], variant=DFMC),
    'sparse': dict(types=TWO, relations=[rel(SPARSE, known=10)]),
    'sparse-fill': dict(types=TWO, relations=[rel(SPARSE | RANK1, known=10)], variant=DFMC),
    'fold': dict(types=TWO, relations=[rel(FOLD, known=10)], variant=TRANSFORM, target=0),
    'fold-column-side': dict(types=TWO, relations=[rel(FOLD, known=10)], variant=TRANSFORM, target=1),
    'fold-known': dict(types=TWO, relations=[rel(FOLD | FOLD_KNOWN, known=10)], variant=TRANSFORM, target=0),
    'fold-dense-target-2': dict(types=THREE, relations=[rel(col=2, cols=20)], variant=TRANSFORM, target=2),
    'row-block': dict(types=TWO, relations=[rel(begin=20, rows=20)], part=(1, 2)),
    'row-block-bf16': dict(types=TWO64, relations=[rel(begin=64, rows=64, cols=64)], dtype=BF16, part=(1, 2)),
    'absent': dict(types=TWO, relations=[rel(ABSENT | NO_COL)], part=(0, 2)),
    'owned': dict(types=TWO, relations=[rel(rows=20)], part=(0, 2), opt_flags=OWNED),
    'owned-bf16': dict(types=TWO64, relations=[rel(begin=64, rows=64, cols=64)], dtype=BF16, part=(1, 2), opt_flags=OWNED),
    'owned-bf16-absent': dict(types=TWO64, relations=[rel(ABSENT, row=1, col=0)], dtype=BF16, part=(1, 2), opt_flags=OWNED),
    'owned-sparse': dict(types=TWO, relations=[rel(SPARSE, known=10, begin=20, rows=20)], part=(1, 2), opt_flags=OWNED),
    'owned-known-lists': dict(types=TWO, relations=[rel(MASKED | LISTS, rows=20, mask=True, mask_ld=30, known=10)], variant=DFMC,
                              part=(0, 2), opt_flags=OWNED),
    'owned-known-lists-absent': dict(types=TWO64, relations=[rel(ABSENT | MASKED | LISTS, row=1, col=0)], variant=DFMC, dtype=BF16,
                                     part=(1, 2), opt_flags=OWNED),
    'theta-dense': dict(types=TWO, relations=[rel()], thetas=[theta(nnz=10)]),
    'theta-entries': dict(types=TWO, relations=[rel()], thetas=[theta(data=False, nnz=10)]),
    'theta-entries-owned': dict(types=TWO, relations=[rel(rows=20)], thetas=[theta(data=False, nnz=10)], part=(0, 2),
                                opt_flags=OWNED | THETA_OWNED),
    'theta-on-target': dict(types=TWO, relations=[rel(FOLD, known=10)], thetas=[theta()], variant=TRANSFORM, target=0),
}


def refusal_case(lib, name):
    text, kwargs = REFUSALS[name]
    status, said = plan_create_status(lib, **kwargs)
    assert status == BAD, '%s: status %d' % (name, status)
    assert said == text, '%s:\n  said    %r\n  written %r' % (name, said, text)


def null_array_cases(lib):
    """The three refusals that need a NULL where the helper always passes an array."""
    opt = nat.Options(F64, DFMF, -1, MFMA, 0, 0, 0)
    tdesc = (nat.TypeDesc * 2)()
    tdesc[0].n_obj, tdesc[0].rank, tdesc[1].n_obj, tdesc[1].rank = 40, 4, 30, 3
    rdesc, hdesc, handle = (nat.RelationDesc * 1)(), (nat.ThetaDesc * 1)(), nat._P()
    for args, text in (((2, None, 0, None, 0, None, C.byref(opt), C.byref(handle)), 'null argument / no object types'),
                       ((2, tdesc, 0, None, 0, None, None, C.byref(handle)), 'null argument / no object types'),
                       ((2, tdesc, 0, None, 0, None, C.byref(opt), None), 'null argument / no object types'),
                       ((2, tdesc, 1, None, 0, None, C.byref(opt), C.byref(handle)), 'bad relation / constraint arrays'),
                       ((2, tdesc, 0, None, 1, None, C.byref(opt), C.byref(handle)), 'bad relation / constraint arrays'),
                       ((2, tdesc, -1, rdesc, 0, hdesc, C.byref(opt), C.byref(handle)), 'bad relation / constraint arrays'),
                       ((2, tdesc, 0, rdesc, -1, hdesc, C.byref(opt), C.byref(handle)), 'bad relation / constraint arrays'),
                       # a NULL options pointer answers before anything is read through it
                       ((0, tdesc, -1, None, 0, None, None, C.byref(handle)), 'null argument / no object types')):
        assert lib.skf_plan_create(*args) == BAD and not handle.value
        assert lib.skf_last_error().decode() == text


def accepted_case(lib, name):
    status, said = plan_create_status(lib, **ACCEPTED[name])
    assert status == 0, '%s: status %d, %s' % (name, status, said)
