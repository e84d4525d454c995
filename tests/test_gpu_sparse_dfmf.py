"""Relations handed over as the CSR of their stored entries, zero elsewhere (SKF_REL_SPARSE_CSR) on the MI355X: every
valued list pass and the error pass against the host model at the ranks of all list kernels, the lists a bind builds
against scipy.sparse, whole fits against the oracle and against the dense-fed plan, the dicty golden through scipy.sparse
relations, the public API, and a 1 000 000 x 400 000 relation that is never expanded anywhere."""
import resource

import numpy as np
import pytest

import skfusion_amd._native as nat
from helpers import relerr, within

import sparse_dfmf_cases as SC

pytestmark = pytest.mark.gpu

N_A, N_B = 459, 453         # 8 parts of 64 rows / columns, the last one a tail of 11 / 5

# (engine, rank of a = width of the Q gathers, rank of b = width of the P gathers): launch_srp's variants
VARIANTS = [('f64', 16, 128), ('f64', 32, 64), ('f64', 64, 20), ('f64', 128, 16), ('f64', 20, 32),
            ('f32', 32, 256), ('f32', 64, 128), ('f32', 128, 24), ('f32', 256, 32), ('f32', 24, 64),
            ('bf16', 64, 512), ('bf16', 128, 256), ('bf16', 256, 128), ('bf16', 512, 20), ('bf16', 20, 64)]


@pytest.mark.parametrize('parts', [1, 2, 4, 8])
@pytest.mark.parametrize('dtype,rank_a,rank_b', VARIANTS)
def test_valued_passes_and_error_pass_against_host_model(dtype, rank_a, rank_b, parts, monkeypatch):
    for pattern in ('edges', 'full', 'heavy'):
        SC.pass_case(N_A, N_B, rank_a, rank_b, dtype, parts, pattern,
                     'GPU %s ranks %d/%d parts %d %s' % (dtype, rank_a, rank_b, parts, pattern), monkeypatch, seed=parts)


@pytest.mark.parametrize('dtype,parts', [('f64', 1), ('f32', 2), ('bf16', 1), ('bf16', 8)])
def test_bound_lists_equal_scipy_lists(dtype, parts, monkeypatch):
    SC.lists_case(3000, 2600, 128, 64, dtype, parts, 0.02, monkeypatch, seed=parts, edits=('empty', 'full_row'))


def test_bound_lists_of_an_all_zero_relation(monkeypatch):
    SC.lists_case(300, 260, 128, 64, 'bf16', 2, 0.02, monkeypatch, edits=('none',))


@pytest.mark.parametrize('kind', ['indptr', 'column', 'order', 'handover'])
def test_invalid_lists_are_refused_before_any_iteration(kind):
    SC.invalid_lists_case(kind, 'bf16')


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_stored_entries_are_refused_before_any_gather(which):
    SC.refusal_order_case(which)


def test_flag_combinations():
    SC.invalid_flag_cases()


N = {'a': 3000, 'b': 2600, 'c': 500}
# the bounds the list path is held to against the dense path (test_gpu_parity.py, sparse_against_dense): G, S, squared error
TOL = {'f64': (1.5e-12, 6e-12, 1.3e-13), 'f32': (7e-6, 3.5e-5, 1.5e-7), 'bf16': (1.2e-2, 2.5e-2, 5.5e-4)}


@pytest.mark.parametrize('rank_b', [64, 256])
def test_csr_fed_f64_fit_against_the_oracle(rank_b):
    SC.csr_against_oracle(N, {'a': 128, 'b': rank_b, 'c': 64}, 10, 1e-9, 'GPU rank_b %d' % rank_b)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
@pytest.mark.parametrize('rank_b', [64, 128, 256])
def test_csr_fed_fit_against_dense_fed_fit(dtype, rank_b):
    SC.csr_against_dense(N, {'a': 128, 'b': rank_b, 'c': 64}, dtype, TOL[dtype], 'GPU %s rank_b %d' % (dtype, rank_b))


@pytest.mark.parametrize('kw', [dict(zero_rel=True), dict(empty_side=True)])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_all_zero_relation_and_empty_side(dtype, kw):
    SC.csr_against_dense(N, {'a': 128, 'b': 64, 'c': 64}, dtype, TOL[dtype], 'GPU %s %s' % (dtype, sorted(kw)), **kw)


def test_csr_fed_dfmc_unmasked_relations():
    """Unmasked relations of a DFMC plan take the same lists.  Bounds: the ones DFMC's list path is held to against its dense
    path in f64 (test_gpu_known_csr.py, forced lists against the dense completion: G 5e-12, S 1.2e-11, squared error 3e-13)."""
    SC.csr_against_dense(N, {'a': 128, 'b': 64, 'c': 64}, 'f64', (5e-12, 1.2e-11, 3e-13), 'GPU DFMC', variant=nat.SKF_DFMC)


def test_dicty_golden_through_scipy_sparse_relations():
    """BASELINE config 2 (ranks 50 / 15 / 5: the staged schedule, never the small-graph one) with both relations handed over
    as scipy.sparse matrices and taken as their stored entries -- the dense-valued expression relation included -- against
    the golden, within the 5e-9 the ndarray form is held to (test_gpu_parity.py)."""
    import scipy.sparse
    from helpers import golden, dicty_graph, g0_from, Snapshots, compare_snapshots
    from skfusion_amd.fusion import Relation, ObjectType
    from skfusion_amd.fusion.decomposition import _dfmf
    from skfusion_amd.fusion.decomposition.dfmf import stored_entries_apply
    from oracle import dfmf_oracle as orc
    z = golden('c2_dicty.npz')
    R, Theta, types, rank = dicty_graph()
    ot = {t: ObjectType(t, rank[t]) for t in types}
    Rs = {}
    for (i, j), mats in R.items():
        rel = Relation(scipy.sparse.csr_matrix(mats[0]), ot[i], ot[j])
        assert stored_entries_apply(rel, True)
        Rs[i, j] = [rel.stored_entries()]
    snaps = Snapshots((0, 9, 99))
    G, S = _dfmf.dfmf(Rs, Theta, types, rank, max_iter=100, callback=snaps, G0=g0_from(z, 'dfmf/', types), dtype='f64')
    within(compare_snapshots(z, 'dfmf/', snaps.snap, 5e-9), 5e-9, 'dicty f64 dfmf through scipy.sparse relations vs golden')
    errs = orc.relation_errors(R, G, S)
    for (i, j), e in errs.items():
        assert relerr(e, z['dfmf/err_%s_%s' % (i, j)]) < 1e-9


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_api_eligible_relation_is_never_expanded(dtype, monkeypatch):
    import sparse_dfmf_api_cases as AC
    from skfusion_amd.fusion import Dfmf
    AC.eligible_case(Dfmf, dtype, (900, 700), monkeypatch, ranks=(128, 64, 32), n_g=200, init_type='random')


def test_api_dfmc_and_everything_else(monkeypatch, tmp_path):
    import sparse_dfmf_api_cases as AC
    from skfusion_amd.fusion import Dfmf, Dfmc
    AC.eligible_case(Dfmc, 'f64', (900, 700), monkeypatch, ranks=(128, 64, 32), n_g=200, init_type='random')
    AC.ineligible_cases(Dfmf, 'f64', (300, 250))
    for init_type in ('random_c', 'random_vcol'):
        AC.initialiser_case((600, 500), init_type)
    AC.stopping_case((600, 500))
    AC.restarts_case((600, 500), 'f64', monkeypatch)
    AC.complete_save_load_case((300, 250), 'f64', tmp_path)


def _peak_rss_bytes():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024


def test_million_by_400k_relation_is_never_densified():
    """1 000 000 x 400 000, 40 entries per row (40 M), ranks 128 / 64, bf16 engine, three iterations.  Derived, not
    measured: lists 40 M x (4 + 4) B x 2 + pointers ~ 0.7 GB; the n x c masters G, E, D, P, Q, H and the bf16 copies of G
    ~ 3.5 GB -- workspace < 8 GiB (the dense bf16 relation alone would be 800 GB); the host holds the CSR (0.5 GB) and
    the factors: peak RSS growth < 4 GiB."""
    from skfusion_amd._engine import DevicePlan, KnownEntries
    n_r, n_c, per_row = 1000000, 400000, 40
    rss0 = _peak_rss_bytes()
    rs = np.random.RandomState(0)
    step = n_c // per_row
    cols = rs.randint(0, step, (n_r, per_row), dtype=np.int32)
    cols += (np.arange(per_row, dtype=np.int32) * step)[None, :]                   # strictly ascending in every row
    vals = rs.randint(1, 64, n_r * per_row, dtype=np.int32).astype(np.float64)
    vals /= 8.0
    ke = KnownEntries(np.arange(n_r + 1, dtype=np.int64) * per_row, cols.reshape(-1), vals, (n_r, n_c), unstored='zero')
    del cols, vals
    types, n, rank = ['row', 'col'], {'row': n_r, 'col': n_c}, {'row': 128, 'col': 64}
    plan = DevicePlan(types, n, rank, [('row', 'col', ke, None)], [], nat.SKF_DFMF, dtype='bf16')
    try:
        assert plan.workspace_bytes < 8 * 2 ** 30, plan.workspace_bytes
        for t in types:
            plan.set_factor(t, (rs.rand(n[t], rank[t]) * 0.1 + 0.01).astype(np.float32))
        errs = []
        for _ in range(3):
            plan.iterate(1)
            errs.append(plan.relation_sqerr(0))
        finite = all(bool(np.isfinite(plan.get_factor(t)).all()) for t in types)
    finally:
        plan.close()
    assert finite
    assert np.isfinite(errs).all() and errs[2] < errs[1] < errs[0], errs
    grew = _peak_rss_bytes() - rss0
    assert grew < 4 * 2 ** 30, 'host peak RSS grew by %.2f GB' % (grew / 2 ** 30)
