"""Ranks of held-out pairs on the GPU (tests/ranks_cases.py): exact lattice cases at every shape with P1 against the top-k
operator, the random cases within their derived interval, NaN, refusals, the public API, and the ranks of a million pairs of
a 200 000 x 400 000 completion that is never densified."""
import resource

import numpy as np
import pytest

import complete_cases as CC
import ranks_cases as RC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('ranks', [(5, 1), (5, 7), (64, 65), (128, 128)])
@pytest.mark.parametrize('n_cols', [7, 203, 997])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_count_for_count_bit_for_bit(dtype, n_cols, ranks):
    for m in (67, 131):
        RC.exact_case(dtype, m, n_cols, ranks)


@pytest.mark.parametrize('pattern', ['none', 'edges', 'heavy'])
@pytest.mark.parametrize('ranks', [(20, 64), (128, 200), (128, 256)])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_random_within_the_derived_interval(dtype, ranks, pattern):
    RC.random_case(dtype, ranks, pattern=pattern, label='gpu')


def test_bf16_name_scores_on_the_f32_masters():
    a, b = RC.random_case('f32', (20, 64)), RC.random_case('bf16', (20, 64))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "the 'bf16' engine name must score on the f32 masters"


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_scores(dtype):
    RC.nan_case(dtype)


def test_refusals():
    RC.refusals_case('f64')
    RC.refusals_case('f32')


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, dtype, monkeypatch):
    RC.api_case(kind, dtype, monkeypatch)


def test_public_api_runs():
    RC.api_runs_case()


def test_200k_by_400k_is_never_densified():
    """DeviceCompleter.ranks, f32 random factors, 200 000 x 400 000, rank 16, every row in blocks of 8192 with 5 targets and
    40 excluded columns per row (1 M pairs ranked against 8 M exclusions).  The dense f32 score matrix would be 320 GB.

    device_bytes < 256 MiB, derived: G_col 400 000 x 16 x 4 B = 25.6 MB and S; per block the uploaded rows and H (2 x 0.5 MB),
    the target slice (8192 x 5 x 4 B + pointers = 0.23 MB), the exclusion slice (8192 x 40 x 4 B + pointers = 1.4 MB), one
    rank and one score per pair (40 960 x 8 B = 0.33 MB) and a workspace of 512 B of flag words plus 40 960 scores (0.16 MB):
    under 30 MB, an eighth of the limit -- there are no partial lists, the splits meet in integer atomics.  Host peak RSS may
    grow by < 1 GiB: the lists take 0.1 GB, the results 1 M x 12 B, the row factor 13 MB.  On a fixed sample of 16 rows the
    random-case conditions hold in float64: every rank inside its derived interval, every value within its bound."""
    from skfusion_amd._engine import DeviceCompleter
    n_i, n_j, c, per_tgt, per_row, block = 200000, 400000, 16, 5, 40, 8192
    rs = np.random.RandomState(0)
    G_row = (rs.rand(n_i, c) * 0.1 + 0.01).astype(np.float32)
    S = (rs.rand(c, c) * 0.2).astype(np.float32)
    G_col = (rs.rand(n_j, c) * 0.1 + 0.01).astype(np.float32)
    # ascending columns per row: one in every stride of n_j / 40 (exclusion) resp. n_j / 5 (targets)
    stride = n_j // per_row
    excl = (rs.randint(0, stride, size=(n_i, per_row)) + np.arange(per_row) * stride).astype(np.int32)
    tstride = n_j // per_tgt
    tgt = (rs.randint(0, tstride, size=(n_i, per_tgt)) + np.arange(per_tgt) * tstride).astype(np.int32)
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    comp = DeviceCompleter(S, G_col, dtype='f32')
    rank = np.empty((n_i, per_tgt), dtype=np.int32)
    val = np.empty((n_i, per_tgt), dtype=np.float64)
    for r0 in range(0, n_i, block):
        r1 = min(r0 + block, n_i)
        steps = np.arange(r1 - r0 + 1, dtype=np.int64)
        rk, vl = comp.ranks(G_row[r0:r1], (steps * per_tgt, tgt[r0:r1].reshape(-1)), exclude=(steps * per_row, excl[r0:r1].reshape(-1)))
        rank[r0:r1], val[r0:r1] = rk.reshape(-1, per_tgt), vl.reshape(-1, per_tgt)
    grown = (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before) * 1024
    assert comp.peak_bytes >= comp.device_bytes > 0
    assert comp.peak_bytes < 256 * 2 ** 20, 'the completer held %.1f MiB in HBM' % (comp.peak_bytes / 2.0 ** 20)
    assert grown < 2 ** 30, 'host peak RSS grew by %.2f GiB' % (grown / 2.0 ** 30)
    assert (rank >= 0).all() and (rank < n_j).all()
    sample = np.random.RandomState(1).choice(n_i, 16, replace=False)
    Gr, S64, Gc = G_row[sample].astype(np.float64), S.astype(np.float64), G_col.astype(np.float64)
    X64 = np.dot(np.dot(Gr, S64), Gc.T)
    B = CC.bound(Gr, S64, Gc, 'f32')
    ex = np.zeros((16, n_j), dtype=bool)
    ex[np.repeat(np.arange(16), per_row), excl[sample].reshape(-1)] = True
    tl = (np.arange(17, dtype=np.int64) * per_tgt, tgt[sample].reshape(-1))
    RC.check_random(rank[sample].reshape(-1), val[sample].reshape(-1), tl, X64, B, ex, 'never densified')
