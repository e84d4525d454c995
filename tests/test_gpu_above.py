"""Scores at or above a threshold as CSR on the GPU (tests/above_cases.py): exact lattice cases at every shape, P2 against the
top-k operator and the agreement with the rank operator, the random cases under their derived bound, NaN, refusals, the public
API, and the pairs above a per-row threshold of a 100 000 x 400 000 completion that is never densified."""
import resource

import numpy as np
import pytest

import complete_cases as CC
import above_cases as AC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('ranks', [(5, 1), (5, 7), (64, 65), (128, 128)])
@pytest.mark.parametrize('n_cols', [7, 203, 997])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_index_for_index_bit_for_bit(dtype, n_cols, ranks):
    for m in (67, 131):
        AC.exact_case(dtype, m, n_cols, ranks)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exclusion_entries_on_either_side_of_a_split_boundary(dtype):
    AC.seam_case(dtype)


@pytest.mark.parametrize('m', [600, 262144 + 300])
def test_scan_over_several_chunks_of_rows(m):
    """600 rows: three workgroups of the scan; 262 444 rows: 513 workgroups that walk 512 rows each in two steps."""
    AC.scan_case('f32', m)
    if m == 600:
        AC.scan_case('f64', m, col_splits=1)


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_exclusion_lists_are_refused_before_any_gather(which):
    AC.refusal_order_case(which)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_agrees_with_topk_and_ranks(dtype):
    assert AC.agreement_case(dtype, 131, 997, (5, 7)) > 0            # rank 5: ties beyond the k-th entry exist
    AC.agreement_case(dtype, 67, 7, (5, 1), pattern='none')
    AC.agreement_case(dtype, 67, 203, (64, 65), pattern='heavy')
    AC.agreement_case(dtype, 131, 997, (128, 200), pattern='heavy', factors=AC.random_factors)


@pytest.mark.parametrize('pattern', ['none', 'edges', 'heavy'])
@pytest.mark.parametrize('ranks', [(5, 7), (20, 64), (128, 200), (128, 256)])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_random_under_the_derived_bound(dtype, ranks, pattern):
    AC.random_case(dtype, ranks, pattern=pattern, label='gpu')
    if pattern == 'edges':
        AC.random_case(dtype, ranks, m=67, n_cols=203, pattern=pattern, label='gpu')


def test_bf16_name_scores_on_the_f32_masters():
    a, b = AC.random_case('f32', (20, 64)), AC.random_case('bf16', (20, 64))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "the 'bf16' engine name must score on the f32 masters"


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_scores(dtype):
    AC.nan_case(dtype)


def test_refusals():
    AC.refusals_case('f64')
    AC.refusals_case('f32')


@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, monkeypatch):
    AC.api_case(kind, monkeypatch)


def test_public_api_runs():
    AC.api_runs_case()


def test_100k_by_400k_is_never_densified():
    """DeviceCompleter.above, f32 random factors, 100 000 x 400 000, rank 16, every row in blocks of 8192 with 40 excluded
    columns per row; thr is the 8th value of DeviceCompleter.topk of the same block.  The dense f32 score matrix would be
    160 GB.

    peak_bytes < 256 MiB, derived: G_col 400 000 x 16 x 4 B = 25.6 MB and S; per block the uploaded rows and H (2 x 0.5 MB),
    the thresholds (32 KB), the exclusion slice (8192 x 40 x 4 B + pointers = 1.4 MB); of top-k the lists (8192 x 8 x 8 B =
    0.5 MB) and the partial lists of its 4 column splits (2 MB); of this operator the pointers (64 KB), room for 64 entries
    per row (8192 x 64 x 8 B = 4 MB: a row holds 8 entries plus ties, the first call suffices) and a workspace of 8.4 KB of
    flag and scan words plus 4 x 8192 int64 (0.26 MB): under 40 MB, a sixth of the limit.  Host peak RSS may grow by < 1 GiB:
    the lists take 16 MB, the row factor 6 MB, the result about 0.8 M entries x 12 B.  Every row holds at least 8 entries; on a
    fixed sample of 16 rows P2 holds against the device's own top-k and the random-case conditions hold in float64."""
    from skfusion_amd._engine import DeviceCompleter
    n_i, n_j, c, per_row, block, k = 100000, 400000, 16, 40, 8192, 8
    rs = np.random.RandomState(0)
    G_row = (rs.rand(n_i, c) * 0.1 + 0.01).astype(np.float32)
    S = (rs.rand(c, c) * 0.2).astype(np.float32)
    G_col = (rs.rand(n_j, c) * 0.1 + 0.01).astype(np.float32)
    stride = n_j // per_row                      # ascending columns per row: one in every stride of n_j / 40
    excl = (rs.randint(0, stride, size=(n_i, per_row)) + np.arange(per_row) * stride).astype(np.int32)
    sample = np.sort(np.random.RandomState(1).choice(n_i, 16, replace=False))
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    comp = DeviceCompleter(S, G_col, dtype='f32')
    counts = np.empty(n_i, dtype=np.int64)
    kept = {}                                    # sample row -> (its top-k list, its threshold, its entries)
    for r0 in range(0, n_i, block):
        r1 = min(r0 + block, n_i)
        xl = (np.arange(r1 - r0 + 1, dtype=np.int64) * per_row, excl[r0:r1].reshape(-1))
        ti, tv = comp.topk(G_row[r0:r1], k, exclude=xl)
        thr = tv[:, k - 1]
        p, i, v = comp.above(G_row[r0:r1], thr, exclude=xl)
        counts[r0:r1] = np.diff(p)
        for r in sample[(sample >= r0) & (sample < r1)]:
            q = r - r0
            kept[r] = (ti[q], tv[q], thr[q], i[p[q]:p[q + 1]], v[p[q]:p[q + 1]])
    grown = (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before) * 1024
    assert comp.peak_bytes >= comp.device_bytes > 0
    assert comp.peak_bytes < 256 * 2 ** 20, 'the completer held %.1f MiB in HBM' % (comp.peak_bytes / 2.0 ** 20)
    assert grown < 2 ** 30, 'host peak RSS grew by %.2f GiB' % (grown / 2.0 ** 30)
    assert (counts >= k).all(), 'a row holds fewer than %d entries' % k
    ti = np.stack([kept[r][0] for r in sample])
    tv = np.stack([kept[r][1] for r in sample])
    thr = np.array([kept[r][2] for r in sample])
    p = np.zeros(17, dtype=np.int64)
    np.cumsum([kept[r][3].size for r in sample], out=p[1:])
    got = (p, np.concatenate([kept[r][3] for r in sample]), np.concatenate([kept[r][4] for r in sample]))
    AC.check_p2(got, ti, tv, thr, k, 'never densified P2')
    Gr, S64, Gc = G_row[sample].astype(np.float64), S.astype(np.float64), G_col.astype(np.float64)
    X64 = np.dot(np.dot(Gr, S64), Gc.T)
    B = CC.bound(Gr, S64, Gc, 'f32')
    ex = np.zeros((16, n_j), dtype=bool)
    ex[np.repeat(np.arange(16), per_row), excl[sample].reshape(-1)] = True
    AC.check_random(got, X64, B, thr.astype(np.float32), ex, 'never densified')
