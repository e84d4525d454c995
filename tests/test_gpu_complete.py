"""Top-k completion and entry predictions on the GPU (tests/complete_cases.py): exact lattice cases at every shape, the
random cases within their derived bound, refusals, the public API, and a 200 000 x 400 000 completion that is never
densified."""
import resource

import numpy as np
import pytest

import complete_cases as CC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('ranks', [(5, 1), (5, 7), (64, 65), (128, 128)])
@pytest.mark.parametrize('n_cols', [7, 203, 997])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_index_for_index_bit_for_bit(dtype, n_cols, ranks):
    for m in (67, 131):
        CC.exact_case(dtype, m, n_cols, ranks)


@pytest.mark.parametrize('pattern', ['none', 'edges', 'heavy'])
@pytest.mark.parametrize('ranks', [(20, 64), (128, 200), (128, 256)])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_random_within_the_derived_bound(dtype, ranks, pattern):
    CC.random_case(dtype, ranks, pattern=pattern, label='gpu')
    print('largest |out_val - X64| / b so far: %r' % (CC.WORST,))


def test_bf16_name_scores_on_the_f32_masters():
    CC.bf16_is_f32_case()


def test_refusals():
    CC.refusals_case('f64')
    CC.refusals_case('f32')


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_exclusion_lists_are_refused_before_any_gather(which):
    CC.refusal_order_case(which)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, dtype, monkeypatch):
    CC.api_case(kind, dtype, monkeypatch)


def test_public_api_runs():
    CC.api_runs_case()


def test_200k_by_400k_is_never_densified():
    """DeviceCompleter, f32 random factors, 200 000 x 400 000, rank 16, k = 8, every row in blocks of 8192, 40 excluded
    columns per row (8 M entries).  The dense f32 score matrix would be 320 GB.

    device_bytes < 256 MiB, derived: G_col 400 000 x 16 x 4 B = 25.6 MB and S; per block the uploaded rows and H (2 x 0.5 MB),
    the outputs (8192 x 8 x (4 + 4) B = 0.5 MB), the partial lists of at most 32 column splits (32 x 0.5 MB = 16.8 MB), the
    exclusion slice (8192 x 40 x 4 B + pointers = 1.4 MB): under 50 MB, a fifth of the limit, and 1/6000 of the dense form.
    Host peak RSS may grow by < 1 GiB: the lists take 0.1 GB, the results 200 000 x 8 x 12 B = 19 MB, the row factor 13 MB.
    No excluded column may come back, and the random-case conditions hold on a fixed sample of 16 rows in float64."""
    from skfusion_amd._engine import DeviceCompleter
    n_i, n_j, c, k, per_row, block = 200000, 400000, 16, 8, 40, 8192
    rs = np.random.RandomState(0)
    G_row = (rs.rand(n_i, c) * 0.1 + 0.01).astype(np.float32)
    S = (rs.rand(c, c) * 0.2).astype(np.float32)
    G_col = (rs.rand(n_j, c) * 0.1 + 0.01).astype(np.float32)
    # 40 ascending columns per row: one in every stride of n_j / 40
    stride = n_j // per_row
    excl = (rs.randint(0, stride, size=(n_i, per_row)) + np.arange(per_row) * stride).astype(np.int32)
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    comp = DeviceCompleter(S, G_col, dtype='f32')
    idx = np.empty((n_i, k), dtype=np.int32)
    val = np.empty((n_i, k), dtype=np.float64)
    for r0 in range(0, n_i, block):
        r1 = min(r0 + block, n_i)
        indptr = np.arange(r1 - r0 + 1, dtype=np.int64) * per_row
        idx[r0:r1], val[r0:r1] = comp.topk(G_row[r0:r1], k, exclude=(indptr, excl[r0:r1].reshape(-1)))
    grown = (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before) * 1024
    assert comp.peak_bytes >= comp.device_bytes > 0
    assert comp.peak_bytes < 256 * 2 ** 20, 'the completer held %.1f MiB in HBM' % (comp.peak_bytes / 2.0 ** 20)
    assert grown < 2 ** 30, 'host peak RSS grew by %.2f GiB' % (grown / 2.0 ** 30)
    assert (idx >= 0).all() and (idx < n_j).all()
    hit = (idx[:, :, None] == excl[:, None, :]).any()
    assert not hit, 'an excluded column came back'
    sample = np.random.RandomState(1).choice(n_i, 16, replace=False)
    Gr, S64, Gc = G_row[sample].astype(np.float64), S.astype(np.float64), G_col.astype(np.float64)
    X64 = np.dot(np.dot(Gr, S64), Gc.T)
    B = CC.bound(Gr, S64, Gc, 'f32')
    ex = np.zeros((16, n_j), dtype=bool)
    ex[np.repeat(np.arange(16), per_row), excl[sample].reshape(-1)] = True
    worst = CC.check_conditions(idx[sample], val[sample], X64, B, ex, k, 'never densified')
    CC.WORST['f32'] = max(CC.WORST.get('f32', 0.0), worst)
