"""The n best pairs of a whole relation on the GPU (tests/best_cases.py): exact lattice cases at every shape, the raw
histograms against the host's keys, P3 against the above operator, a single row against top-k, the random cases under their
derived bound, NaN and infinities, independence of blocks and splits, refusals, the public API, and the 100 000 best pairs of
a 100 000 x 400 000 completion that is never densified."""
import resource

import numpy as np
import pytest

import complete_cases as CC
import best_cases as BC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('ranks,signed', [((5, 1), False), ((5, 7), False), ((64, 65), False), ((5, 7), True), ((5, 1), True)])
@pytest.mark.parametrize('n_cols', [7, 203, 997])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_index_for_index_bit_for_bit(dtype, n_cols, ranks, signed):
    ties = 0
    for m in (67, 131):
        ties += BC.exact_case(dtype, m, n_cols, ranks, signed=signed)
    assert ties > 0 or ranks != (5, 1), 'no tie class larger than what is wanted of it is exercised'


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exclusion_entries_on_either_side_of_a_split_boundary(dtype):
    BC.seam_case(dtype)


@pytest.mark.parametrize('signed', [False, True])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_every_pass_is_the_bincount_of_the_host_keys(dtype, signed):
    BC.digits_case(dtype, 131, 997, (5, 7), signed=signed, pattern='heavy')
    BC.digits_case(dtype, 67, 203, (64, 65), signed=signed)
    BC.digits_case(dtype, 67, 7, (5, 1), signed=signed, pattern='none')


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_exclusion_lists_are_refused_before_anything_is_counted(which):
    BC.refusal_order_case(which)


def test_refusals():
    BC.refusals_case('f64')
    BC.refusals_case('f32')


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_p3_and_agreement_with_above_and_ranks(dtype):
    assert BC.agreement_case(dtype, 131, 997, (5, 7), ns=(1, 64, 1000, 5000)) > 0      # rank 5: ties at the n-th score exist
    BC.agreement_case(dtype, 67, 7, (5, 1), pattern='none', ns=(1, 64))
    BC.agreement_case(dtype, 67, 203, (64, 65), pattern='heavy')
    BC.agreement_case(dtype, 131, 997, (128, 200), pattern='heavy', factors=BC.random_factors, ns=(2000,))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_single_row_is_topk(dtype):
    BC.single_row_case(dtype, 997, (5, 7))
    BC.single_row_case(dtype, 203, (20, 64), pattern='heavy', factors=BC.random_factors)
    BC.single_row_case(dtype, 7, (5, 1), pattern='none')


@pytest.mark.parametrize('ranks', [(5, 7), (20, 64), (128, 200), (128, 256)])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_random_under_the_derived_bound(dtype, ranks):
    BC.random_case(dtype, ranks, label='gpu')
    if ranks == (20, 64):
        BC.random_case(dtype, ranks, m=67, n_cols=203, n=300, label='gpu')


def test_random_deviations_are_reported():
    """(runs after the random cases: their lines, as profiles/best_pairs.txt records them)"""
    print('\n'.join(BC.DEVIATIONS))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_and_infinities(dtype):
    BC.nan_inf_case(dtype)


def test_independent_of_blocks_splits_and_the_bf16_name():
    a = BC.independence_case('f32')
    assert BC.independence_case('bf16') == a, "the 'bf16' engine name must score on the f32 masters"
    BC.independence_case('f64')


def test_a_tie_class_straddles_two_row_blocks():
    """The (5, 1) lattice at 131 x 997 has 220 distinct scores: the first tie class, from the top, whose pairs lie in more than
    one block of 64 rows, and in it an n whose quota runs out in the class's first block, one that runs out in its last
    block, the whole class and one pair more."""
    G_row, S, G_col = BC.lattice_factors(131, 997, (5, 1))
    X = np.dot(np.dot(G_row, S), G_col.T)
    order = BC.host_order(X)
    rows, vals = order[0], order[2]
    for v in np.unique(vals)[::-1]:
        cls = np.nonzero(vals == v)[0]                               # (contiguous in the order, by rows within the class)
        per_block = np.bincount(rows[cls] // 64, minlength=3)
        if (per_block > 1).sum() > 1:
            break
    else:
        raise AssertionError('no tie class straddles two row blocks')
    g, e = int(cls[0]), int(cls.size)
    first = int(per_block[np.nonzero(per_block)[0][0]])
    fit, rel = BC.model(G_row, S, G_col)
    for n in (g + 1, g + first - 1, g + first, g + first + 1, g + e - 1, g + e, g + e + 1):
        for step in (64, 8192):
            BC.same_csr(fit.complete_best(rel, n, dtype='f32', block_rows=step), BC.host_best(order, n, X.shape), 'tie class n %d' % n)


@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, monkeypatch):
    BC.api_case(kind, monkeypatch)


def test_public_api_runs():
    BC.api_runs_case()


def test_100k_by_400k_is_never_densified(monkeypatch):
    """FusionFit.complete_best, f32 random factors, 100 000 x 400 000, rank 16, 40 excluded columns per row, n = 100 000, blocks
    of 8192: the operands of test_gpu_above.test_100k_by_400k_is_never_densified.  The dense f32 score matrix would be 160 GB.

    peak_bytes < 256 MiB, derived as there: G_col 400 000 x 16 x 4 B = 25.6 MB and S; per block the uploaded rows and H
    (2 x 0.5 MB), the thresholds (32 KB), the exclusion slice (8192 x 40 x 4 B + pointers = 1.4 MB), the pointers (64 KB), room
    for 64 entries per row (8192 x 64 x 8 B = 4 MB; a block holds about 8200 of the 100 000 entries) and a workspace of 8.4 KB
    of flag and scan words plus 4 x 8192 int64 (0.26 MB); the histogram adds 16 KB: under 40 MB, a sixth of the limit.  Host
    peak RSS may grow by < 1 GiB: the exclusion matrix takes 50 MB, the row factor 6 MB, the result 100 000 entries x 12 B.
    Exactly n entries, the smallest of them the threshold of complete_kth; on a fixed sample of 16 rows (8 at random, the 8
    with the largest row sums of G_row S) the random-case conditions hold in float64 against that threshold.  Seven walks over
    the score tiles (three digit passes, two counts, count and fill); well under a second on the MI355X at the full size."""
    import scipy.sparse
    from skfusion_amd._engine import DeviceCompleter
    n_i, n_j, c, per_row, block, n = 100000, 400000, 16, 40, 8192, 100000
    rs = np.random.RandomState(0)
    G_row = (rs.rand(n_i, c) * 0.1 + 0.01).astype(np.float32)
    S = (rs.rand(c, c) * 0.2).astype(np.float32)
    G_col = (rs.rand(n_j, c) * 0.1 + 0.01).astype(np.float32)
    stride = n_j // per_row                      # ascending columns per row: one in every stride of n_j / 40
    excl = (rs.randint(0, stride, size=(n_i, per_row)) + np.arange(per_row) * stride).astype(np.int32)
    xs = scipy.sparse.csr_matrix((np.ones(excl.size, dtype=np.int8), excl.reshape(-1), np.arange(n_i + 1, dtype=np.int64) * per_row),
                                 shape=(n_i, n_j))
    # 16 rows fixed by the inputs alone: 8 at random (one pair in 400 000 is wanted: most rows hold none) and the 8 with
    # the largest sum of H = G_row S, where the best pairs live
    heavy = np.argsort(-np.dot(G_row.astype(np.float64), S.astype(np.float64)).sum(axis=1), kind='stable')[:8]
    sample = np.unique(np.concatenate([np.random.RandomState(1).choice(n_i, 8, replace=False), heavy]))
    assert sample.size == 16
    fit, rel = BC.model(G_row, S, G_col)
    seen = []                                    # (the completer complete_best made, what its selection returned)
    kth = DeviceCompleter.kth

    def recording(self, blocks, n, col_splits=0):
        seen.append((self, kth(self, blocks, n, col_splits)))
        return seen[-1][1]
    monkeypatch.setattr(DeviceCompleter, 'kth', recording)
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    got = fit.complete_best(rel, n, exclude=xs, dtype='f32', block_rows=block)
    grown = (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before) * 1024
    (comp, (T, g, e, cands)), = seen
    assert cands == n_i * (n_j - per_row)
    assert comp.peak_bytes >= comp.device_bytes > 0
    assert comp.peak_bytes < 256 * 2 ** 20, 'the completer held %.1f MiB in HBM' % (comp.peak_bytes / 2.0 ** 20)
    assert grown < 2 ** 30, 'host peak RSS grew by %.2f GiB' % (grown / 2.0 ** 30)
    assert got.shape == (n_i, n_j) and got.nnz == n and got.data.min() == T and g < n <= g + e
    Gr, S64, Gc = G_row[sample].astype(np.float64), S.astype(np.float64), G_col.astype(np.float64)
    X64 = np.dot(np.dot(Gr, S64), Gc.T)
    B = CC.bound(Gr, S64, Gc, 'f32')
    ex = np.zeros((16, n_j), dtype=bool)
    ex[np.repeat(np.arange(16), per_row), excl[sample].reshape(-1)] = True
    sub = got[sample]
    sel = np.zeros((16, n_j), dtype=bool)
    r_of = np.repeat(np.arange(16), np.diff(sub.indptr))
    sel[r_of, sub.indices] = True
    Bm = float(B.max())
    assert not (sel & ex).any(), 'an excluded pair was selected'
    assert sub.nnz > 0 and (np.abs(sub.data - X64[r_of, sub.indices]) <= B[r_of, sub.indices]).all(), 'a value is beyond its bound'
    assert not (~ex & (X64 > T + Bm) & ~sel).any(), 'a pair more than B above the threshold is absent'
    assert not (sel & (X64 < T - Bm)).any(), 'a pair more than B below the threshold is present'
    band = int((~ex & (np.abs(X64 - T) <= 2 * Bm)).sum())
    print('never densified: threshold %.9g, %d above, %d equal, %d entries in the 16 sample rows, %d of %d pairs in the band'
          % (T, g, e, sub.nnz, band, (~ex).sum()))
    assert band <= 0.001 * (~ex).sum()
