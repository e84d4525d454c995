"""Score histograms and ROC / PR curves on the GPU (tests/hist_cases.py): exact lattice cases at every shape, more than 2047
edges in walks, P6 against the above operator for every pair of split counts and P7 against the rank pass, the random cases
under their derived bound, NaN and infinities, independence of blocks and splits, refusals, guard bands, the public API and
the curve, and the histogram of a 100 000 x 400 000 completion that is never densified."""
import resource

import numpy as np
import pytest

import complete_cases as CC
import hist_cases as HC
from guarded import guarded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('ranks,signed', [((5, 1), False), ((5, 7), False), ((64, 65), False), ((5, 7), True)])
@pytest.mark.parametrize('n_cols', [7, 203, 997])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_bin_for_bin(dtype, n_cols, ranks, signed):
    for m in (67, 131):
        HC.exact_case(dtype, m, n_cols, ranks, signed=signed)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_more_than_2047_edges_take_several_walks(dtype):
    HC.walks_case(dtype, 67, 203, n_distinct=2708)
    HC.walks_case(dtype, 131, 997, n_distinct=3808, pattern='heavy')


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_p6_the_bins_above_an_edge_are_above_at_that_threshold(dtype):
    pairs = tuple((a, b) for a in HC.SPLITS for b in HC.SPLITS)
    HC.p6_case(dtype, 131, 997, (5, 7), split_pairs=pairs)
    HC.p6_case(dtype, 67, 7, (5, 1), pattern='none')
    HC.p6_case(dtype, 67, 203, (64, 65), pattern='heavy')
    HC.p6_case(dtype, 131, 203, (5, 7), pattern='heavy', signed=True)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_p7_a_target_lands_in_the_bin_of_its_rank_score(dtype):
    HC.p7_case(dtype, 131, 997, (5, 7))
    HC.p7_case(dtype, 67, 203, (64, 65), pattern='heavy')
    HC.p7_case(dtype, 67, 203, (5, 7), pattern='none', signed=True)


@pytest.mark.parametrize('ranks', [(20, 64), (128, 200)])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_random_under_the_derived_bound(dtype, ranks):
    HC.random_case(dtype, ranks, label='gpu')


def test_random_deviations_are_reported():
    """(runs after the random cases: their lines, as profiles/histogram.txt records them)"""
    print('\n'.join(HC.DEVIATIONS))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_and_infinities(dtype):
    HC.nan_inf_case(dtype)


def test_independent_of_blocks_splits_and_the_bf16_name():
    a = HC.independence_case('f32')
    assert HC.independence_case('bf16') == a, "the 'bf16' engine name must score on the f32 masters"
    HC.independence_case('f64')


def test_refusals():
    HC.refusals_case('f64')
    HC.refusals_case('f32')


def test_refusals_of_the_python_layers():
    HC.python_refusals_case()


def test_between_guard_bands():
    with guarded():
        HC.exact_case('f32', 131, 997, (5, 7), patterns=('heavy',), splits=(0, 3))
    with guarded():
        HC.exact_case('f64', 67, 203, (5, 7), patterns=('edges',), splits=(0, 32), signed=True)
    with guarded():
        HC.refusals_case('f32')


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_curve_counts_and_mid_rank_auroc_exactly(dtype):
    HC.curve_case(dtype)
    HC.curve_case(dtype, m=131, n_cols=997, ranks=(5, 1))
    HC.curve_case(dtype, n_cols=7, ranks=(5, 1), pattern='none')
    HC.curve_case(dtype, pattern='heavy', signed=True)


def test_default_edges_bound_the_float64_auroc():
    HC.default_edges_case()
    HC.default_edges_case(n_cols=997, ranks=(128, 200), pattern='heavy')


@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, monkeypatch):
    HC.api_case(kind, monkeypatch)


def test_public_api_runs():
    HC.api_runs_case()


def test_100k_by_400k_is_never_densified(monkeypatch):
    """FusionFit.complete_histogram, f32 random factors, 100 000 x 400 000, rank 16, 40 excluded columns per row, all rows in
    blocks of 8192, 256 edges, 100 000 random positives: the operands of test_gpu_best.test_100k_by_400k_is_never_densified.
    The dense f32 score matrix would be 160 GB.

    peak_bytes < 256 MiB, derived as there: G_col 400 000 x 16 x 4 B = 25.6 MB and S; per block the uploaded rows and H
    (2 x 0.5 MB), the exclusion slice (8192 x 40 x 4 B + pointers = 1.4 MB) and the block's slice of the targets (about 8200
    pairs: 33 KB + 64 KB of pointers), a workspace of 256 B, 1 KB of edges and 2 x 2 KB of histograms: under 30 MB.  Host peak
    RSS may grow by < 1 GiB: the exclusion matrix takes 50 MB, the row factor 6 MB, the positives 1.2 MB.  Every admissible pair
    is counted once and every positive that is not excluded once; on the sibling's 16 sample rows, run with rows=sample, the
    count at or above every edge lies inside the float64 band of the random case.  One walk over the score tiles."""
    import scipy.sparse
    from skfusion_amd._engine import DeviceCompleter
    import best_cases as BC
    n_i, n_j, c, per_row, block = 100000, 400000, 16, 40, 8192
    rs = np.random.RandomState(0)
    G_row = (rs.rand(n_i, c) * 0.1 + 0.01).astype(np.float32)
    S = (rs.rand(c, c) * 0.2).astype(np.float32)
    G_col = (rs.rand(n_j, c) * 0.1 + 0.01).astype(np.float32)
    stride = n_j // per_row                      # ascending columns per row: one in every stride of n_j / 40
    excl = (rs.randint(0, stride, size=(n_i, per_row)) + np.arange(per_row) * stride).astype(np.int32)
    xs = scipy.sparse.csr_matrix((np.ones(excl.size, dtype=np.int8), excl.reshape(-1), np.arange(n_i + 1, dtype=np.int64) * per_row),
                                 shape=(n_i, n_j))
    heavy = np.argsort(-np.dot(G_row.astype(np.float64), S.astype(np.float64)).sum(axis=1), kind='stable')[:8]
    sample = np.unique(np.concatenate([np.random.RandomState(1).choice(n_i, 8, replace=False), heavy]))
    assert sample.size == 16
    prs = np.random.RandomState(2)
    pr, pc = prs.randint(0, n_i, 100000), prs.randint(0, n_j, 100000)
    pc[:16 * 50] = excl[np.repeat(sample, 50), np.tile(np.arange(50) % per_row, 16)]      # some positives are excluded pairs
    pr[:16 * 50] = np.repeat(sample, 50)
    pos = scipy.sparse.csr_matrix((np.ones(pr.size, dtype=np.int8), (pr, pc)), shape=(n_i, n_j))
    pos.sum_duplicates()
    pos.data[:] = 1
    counted = pos.nnz - pos.multiply(xs).nnz
    assert 0 < counted < pos.nnz <= 100000
    # 256 edges from the scores of the sample rows (float64, then cast to the scoring type by the operator)
    Gr, S64, Gc = G_row[sample].astype(np.float64), S.astype(np.float64), G_col.astype(np.float64)
    X64 = np.dot(np.dot(Gr, S64), Gc.T)
    e = HC.in_type(np.quantile(X64, np.linspace(0.0, 1.0, 256)), 'f32')
    fit, rel = BC.model(G_row, S, G_col)
    seen = []
    histogram = DeviceCompleter.histogram

    def recording(self, blocks, edges, col_splits=0):
        seen.append(self)
        return histogram(self, blocks, edges, col_splits)
    monkeypatch.setattr(DeviceCompleter, 'histogram', recording)
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    counts, tcounts = fit.complete_histogram(rel, e, exclude=xs, targets=pos, dtype='f32', block_rows=block)
    grown = (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before) * 1024
    comp, = seen
    assert int(counts.sum()) == n_i * (n_j - per_row)
    assert int(tcounts.sum()) == counted and (tcounts <= counts).all()
    assert comp.peak_bytes >= comp.device_bytes > 0
    assert comp.peak_bytes < 256 * 2 ** 20, 'the completer held %.1f MiB in HBM' % (comp.peak_bytes / 2.0 ** 20)
    assert grown < 2 ** 30, 'host peak RSS grew by %.2f GiB' % (grown / 2.0 ** 30)
    # the sample rows against float64
    sub, sub_t = fit.complete_histogram(rel, e, rows=sample, exclude=xs, targets=pos, dtype='f32', block_rows=block)
    Bm = float(CC.bound(Gr, S64, Gc, 'f32').max())
    ex = np.zeros((16, n_j), dtype=bool)
    ex[np.repeat(np.arange(16), per_row), excl[sample].reshape(-1)] = True
    tg = np.zeros((16, n_j), dtype=bool)
    p16 = pos[sample].tocoo()
    tg[p16.row, p16.col] = True
    wide = HC.band_check(sub, X64, ~ex, e, Bm, 'never densified, 16 sample rows')
    wide_t = HC.band_check(sub_t, X64, ~ex & tg, e, Bm, 'never densified, 16 sample rows, targets')
    assert (ex & tg).sum() >= 16 * per_row and sub_t.sum() == (~ex & tg).sum() > 0
    print('never densified: %d candidates, %d of %d positives counted, peak %.1f MiB; sample rows: widest band %d of %d, targets %d of %d'
          % (counts.sum(), counted, pos.nnz, comp.peak_bytes / 2.0 ** 20, wide, (~ex).sum(), wide_t, (~ex & tg).sum()))
