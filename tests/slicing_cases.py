"""Plans whose products sit on the edges of the split-K decision (csrc/skf_gemm_launch.inc: slice_gemm): two iterations,
no launch may outgrow the scratch that skf_plan_create sized through the same decision (skf_split_clamps unchanged), the
factors stay finite, and each iteration is held to the host model of tests/dense_cases.py.  The same cases run on the host
emulator (tests/test_slicing_emul.py, EDGES) and on the GPU (tests/test_gpu_slicing.py, EDGES and GPU_ONLY).

Why these shapes (f64 tiles 64 x 128 / 32 x 32 with K tiles of 16, f32 tiles 128 x 128 / 64 x 64 with K tiles of 32; a
product is split only from 32 K tiles on, into at most K tiles / 8 slices):
  gram_ktile_*     496 against 512 objects = 31 against 32 K tiles of G^T G: one slice against four; rank 65 is just past
                   the 64-wide tile and, being odd, has no vector staging: the small tile
  sym_tiles        ranks 192 and 130 on the 64 x 128 tile: 3 x 2 tiles of which the symmetric split computes 4 (rank 192
                   skips a whole tile, rank 130 has a 2-row last tile row)
  group_7_8        1008 against 1040 objects: 63 K tiles give 7 slices, 65 give 8 -- the grouped Gram launch wants 8 of every
                   product and is refused; group_8_8 (1024, 1040): taken
  tile_odd/aligned an f32 relation with 1025 columns (odd leading dimension: no big-tile staging mode, 64 x 64 tile) beside
                   1024 (128 x 128 tile); ranks 68 / 72 are multiples of 4, so only the relation decides
  relation_model_* f32 relations of 4096 and 3968 x 4160: with rank 193 the 64 x 64 tile counts 256 against 248 tiles, the
                   point where the relation time model takes over from the chip-filling one; rank 129 (192 / 186 tiles)
                   stays below it in both"""
import dense_cases as DC
from skfusion_amd._engine import split_clamps

# name: (engine, schedule, object counts, ranks, relations)
EDGES = {
    'gram_ktile_31_32': ('f64', 'pipeline', {'a': 496, 'b': 512}, {'a': 65, 'b': 65}, [('a', 'b', 'neg', None)]),
    'sym_tiles': ('f64', 'pipeline', {'a': 528, 'b': 520}, {'a': 192, 'b': 130}, [('a', 'b', 'neg', None)]),
    'group_7_8': ('f64', 'pipeline', {'a': 1008, 'b': 1040}, {'a': 66, 'b': 68}, [('a', 'b', 'neg', None)]),
    'group_8_8': ('f64', 'pipeline', {'a': 1024, 'b': 1040}, {'a': 66, 'b': 68}, [('a', 'b', 'neg', None)]),
    'tile_odd': ('f32', 'staged', {'a': 200, 'b': 1025}, {'a': 68, 'b': 72}, [('a', 'b', 'neg', None)]),
    'tile_aligned': ('f32', 'staged', {'a': 200, 'b': 1024}, {'a': 68, 'b': 72}, [('a', 'b', 'neg', None)]),
}
GPU_ONLY = {
    'relation_model_4096_r129': ('f32', 'staged', {'a': 4096, 'b': 4160}, {'a': 129, 'b': 129}, [('a', 'b', 'neg', None)]),
    'relation_model_3968_r129': ('f32', 'staged', {'a': 3968, 'b': 4160}, {'a': 129, 'b': 129}, [('a', 'b', 'neg', None)]),
    'relation_model_4096_r193': ('f32', 'staged', {'a': 4096, 'b': 4160}, {'a': 193, 'b': 193}, [('a', 'b', 'neg', None)]),
    'relation_model_3968_r193': ('f32', 'staged', {'a': 3968, 'b': 4160}, {'a': 193, 'b': 193}, [('a', 'b', 'neg', None)]),
}


def slicing_case(case, what, monkeypatch, runtime=None):
    dtype, schedule, n, ranks, rels = case
    before = split_clamps(runtime)
    out = DC.dense_case(dtype, schedule, n, ranks, rels, [], what, monkeypatch, iters=2)      # (asserts finite factors)
    assert split_clamps(runtime) == before, '%s: a launch asked for more slices than its plan sized' % what
    return out
