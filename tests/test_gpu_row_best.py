"""The k best columns of every row for any k on the GPU (tests/row_best_cases.py): exact lattice cases at every shape, P5 against
top-k, P4 against the above operator for every pair of split counts, the rank pass on random factors, NaN and infinities,
independence of blocks and splits, the seam, refusals, guard bands, the public API, and the 200 best columns of 16 384 rows of a
100 000 x 400 000 completion that is never densified."""
import resource

import numpy as np
import pytest

import complete_cases as CC
import best_cases as BC
import row_best_cases as RB
from guarded import guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def no_split_clamps():
    import skfusion_amd._native as nat
    from skfusion_amd._engine import split_clamps
    yield
    assert split_clamps(nat.get_runtime()) == 0


@pytest.mark.parametrize('ranks,signed', [((5, 1), False), ((5, 7), False), ((64, 65), False), ((128, 128), False), ((5, 7), True)])
@pytest.mark.parametrize('n_cols', [7, 203, 997])
@pytest.mark.parametrize('m', [67, 131])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_index_for_index_bit_for_bit(dtype, m, n_cols, ranks, signed):
    trimmed = RB.exact_case(dtype, m, n_cols, ranks, signed=signed)
    assert trimmed > 0 or ranks != (5, 7) or n_cols == 7, 'no row has more pairs at its threshold than are wanted of them'


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_p5_ordered_is_topk(dtype):
    assert RB.p5_case(dtype, 131, 997, (5, 7), pattern='heavy') > 0          # (a row without candidates: the padding)
    RB.p5_case(dtype, 67, 203, (64, 65))
    RB.p5_case(dtype, 67, 7, (5, 1), pattern='none')
    RB.p5_case(dtype, 131, 203, (128, 128), pattern='heavy', factors=BC.random_factors)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_p4_above_at_the_thresholds(dtype):
    assert RB.p4_case(dtype, 131, 997, (5, 7), ks=(1, 65, 100, 'vector')) > 0   # (rows whose threshold is NaN occur)
    RB.p4_case(dtype, 67, 203, (64, 65))
    RB.p4_case(dtype, 67, 7, (5, 1), pattern='none', ks=(1, 9))
    RB.p4_case(dtype, 131, 997, (128, 128), factors=BC.random_factors, ks=(100,))


@pytest.mark.parametrize('shape,ranks', [((67, 203), (20, 64)), ((131, 997), (128, 200))])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_ranks_of_the_selected_pairs(dtype, shape, ranks):
    RB.ranks_case(dtype, m=shape[0], n_cols=shape[1], ranks=ranks)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_and_infinities(dtype):
    RB.nan_inf_case(dtype)


def test_independent_of_blocks_splits_and_the_bf16_name():
    a = RB.independence_case('f32')
    assert RB.independence_case('bf16') == a, "the 'bf16' engine name must score on the f32 masters"
    RB.independence_case('f64', n_cols=997)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exclusion_entries_on_either_side_of_a_split_boundary(dtype):
    RB.seam_case(dtype)


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_exclusion_lists_are_refused_before_anything_is_counted(which):
    RB.refusal_order_case(which)


def test_refusals():
    RB.refusals_case('f64')
    RB.refusals_case('f32')
    RB.engine_refusals_case()


def test_guard_bands():
    """The exact case and the refusals with guard bands around every buffer: no store outside the row histograms, the per-row
    words and the outputs at m = 67."""
    with guarded() as g:
        RB.exact_case('f32', 67, 203, (5, 7))
        RB.exact_case('f64', 67, 997, (64, 65), patterns=('heavy',), ks=(65, 'vector'))
        RB.refusals_case('f64')
    assert g.bands > 0


@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, monkeypatch):
    RB.api_case(kind, monkeypatch)


def test_public_api_runs():
    RB.api_runs_case()


def test_100k_by_400k_is_never_densified(monkeypatch):
    """FusionFit.complete_row_best, f32 random factors, 100 000 x 400 000, rank 16, 40 excluded columns per row (the operands of
    test_gpu_best.test_100k_by_400k_is_never_densified), rows = the first 16 384 row objects, k = 200, blocks of 8192.  The dense
    f32 score block of those rows alone would be 26 GB.

    peak_bytes < 256 MiB, derived as there: G_col 400 000 x 16 x 4 B = 25.6 MB and S; per block the uploaded rows and H
    (2 x 0.5 MB), the wanted counts (64 KB), the exclusion slice (8192 x 40 x 4 B + pointers = 1.4 MB), the select's four
    outputs (32 KB + 3 x 64 KB), the pointers of the fill (64 KB), a workspace of the row histograms 8192 x 2^D x 4 B = 4.2 MB
    (D = 7; 8.4 MB at D = 8) plus two words per row (0.13 MB; the fill's 0.27 MB fit in it) and the entry buffers
    8192 x 200 x 8 B = 13.1 MB plus one entry per row for ties (64 KB; random f32 scores hardly tie): under 52 MB at either
    width, a fifth of the limit.  Host peak RSS may grow
    by < 1 GiB: the exclusion matrix takes 50 MB, the float64 scores and bounds of the 16 sample rows 2 x 51 MB, the result
    16 384 x 200 entries x 12 B = 39 MB.  Every row has exactly 200 entries; on the sample rows no excluded pair is selected,
    every value is within its bound, no unselected admissible pair lies more than the bound above the row's threshold and no
    selected pair more than the bound below it.  Seven walks over the score tiles per block (five digit passes, count, fill)."""
    import scipy.sparse
    from skfusion_amd._engine import DeviceCompleter
    n_i, n_j, c, per_row, block, k, n_rows = 100000, 400000, 16, 40, 8192, 200, 16384
    rs = np.random.RandomState(0)
    G_row = (rs.rand(n_i, c) * 0.1 + 0.01).astype(np.float32)
    S = (rs.rand(c, c) * 0.2).astype(np.float32)
    G_col = (rs.rand(n_j, c) * 0.1 + 0.01).astype(np.float32)
    stride = n_j // per_row                      # ascending columns per row: one in every stride of n_j / 40
    excl = (rs.randint(0, stride, size=(n_i, per_row)) + np.arange(per_row) * stride).astype(np.int32)
    xs = scipy.sparse.csr_matrix((np.ones(excl.size, dtype=np.int8), excl.reshape(-1), np.arange(n_i + 1, dtype=np.int64) * per_row),
                                 shape=(n_i, n_j))
    # the sibling's 16 rows (8 at random, the 8 with the largest sum of H = G_row S), those of them that are asked for
    heavy = np.argsort(-np.dot(G_row.astype(np.float64), S.astype(np.float64)).sum(axis=1), kind='stable')[:8]
    sample = np.unique(np.concatenate([np.random.RandomState(1).choice(n_i, 8, replace=False), heavy]))
    assert sample.size == 16
    sample = sample[sample < n_rows]
    if sample.size == 0:
        sample = np.arange(16)
    fit, rel = BC.model(G_row, S, G_col)
    seen = []                                    # the completers complete_row_best made
    row_best = DeviceCompleter.row_best

    def recording(self, *a, **kw):
        seen.append(self)
        return row_best(self, *a, **kw)
    monkeypatch.setattr(DeviceCompleter, 'row_best', recording)
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    got = fit.complete_row_best(rel, k, rows=np.arange(n_rows), exclude=xs, dtype='f32', block_rows=block)
    grown = (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before) * 1024
    assert len(seen) == n_rows // block and all(s is seen[0] for s in seen)
    comp = seen[0]
    assert comp.peak_bytes >= comp.device_bytes > 0
    assert comp.peak_bytes < 256 * 2 ** 20, 'the completer held %.1f MiB in HBM' % (comp.peak_bytes / 2.0 ** 20)
    assert grown < 2 ** 30, 'host peak RSS grew by %.2f GiB' % (grown / 2.0 ** 30)
    assert got.shape == (n_rows, n_j) and (np.diff(got.indptr) == k).all()
    Gr, S64, Gc = G_row[sample].astype(np.float64), S.astype(np.float64), G_col.astype(np.float64)
    X64 = np.dot(np.dot(Gr, S64), Gc.T)
    B = CC.bound(Gr, S64, Gc, 'f32')
    ns = sample.size
    ex = np.zeros((ns, n_j), dtype=bool)
    ex[np.repeat(np.arange(ns), per_row), excl[sample].reshape(-1)] = True
    sub = got[sample]
    sel = np.zeros((ns, n_j), dtype=bool)
    r_of = np.repeat(np.arange(ns), np.diff(sub.indptr))
    sel[r_of, sub.indices] = True
    thr = np.minimum.reduceat(sub.data, sub.indptr[:-1])[:, None]           # the row's k-th score: the smallest of its k entries
    Bm = float(B.max())
    assert not (sel & ex).any(), 'an excluded pair was selected'
    assert (np.abs(sub.data - X64[r_of, sub.indices]) <= B[r_of, sub.indices]).all(), 'a value is beyond its bound'
    assert not (~ex & (X64 > thr + Bm) & ~sel).any(), 'a pair more than the bound above its row\'s threshold is absent'
    assert not (sel & (X64 < thr - Bm)).any(), 'a pair more than the bound below its row\'s threshold is present'
    print('never densified: %d sample rows, peak %.1f MiB in HBM, host RSS grew by %.2f GiB'
          % (ns, comp.peak_bytes / 2.0 ** 20, grown / 2.0 ** 30))
