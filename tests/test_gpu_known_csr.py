"""Relations handed over as their known entries (SKF_REL_KNOWN_CSR) on the MI355X: bit for bit the mask form's lists at
the sizes and ranks of the list kernels, the forced list path against the dense completion, the config-5 golden, the
public API, and the full config-5 shape built from triplets without any n_i x n_j allocation."""
import resource

import numpy as np
import pytest

import skfusion_amd._native as nat
from helpers import relerr, within

import known_cases as K
import known_csr_cases as KC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
@pytest.mark.parametrize('rank_a', [64, 128, 256])
def test_csr_fed_lists_equal_mask_fed_lists(dtype, rank_a, monkeypatch):
    n, ranks = {'a': 3000, 'b': 2600, 'c': 500}, {'a': rank_a, 'b': 256 if rank_a < 256 else 128, 'c': 64}
    KC.csr_against_mask(n, ranks, 0.02, dtype, 1, monkeypatch)


@pytest.mark.parametrize('rank_a,parts', [(128, 2), (128, 8), (256, 4), (64, 8)])
def test_csr_fed_lists_in_parts_equal_mask_fed_lists(rank_a, parts, monkeypatch):
    """The parted forms of the bf16 list kernels (srp_bf16_v6_kernel pinned to XCDs)."""
    n, ranks = {'a': 3000, 'b': 2600, 'c': 500}, {'a': rank_a, 'b': 128, 'c': 64}
    KC.csr_against_mask(n, ranks, 0.02, 'bf16', parts, monkeypatch, seed=2, edits=('empty', 'full_row'))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_forced_lists_against_the_dense_completion(dtype, monkeypatch):
    """30 % known: the mask form keeps the dense completion, the CSR form can only take the lists -- held to each other
    with the tolerances of the list path against the dense path (test_gpu_parity, known entries)."""
    monkeypatch.delenv('SKF_DFMC_SPARSE', raising=False)
    n, ranks = {'a': 1500, 'b': 1300, 'c': 300}, {'a': 128, 'b': 64, 'c': 32}
    types, rels, thetas, G0 = K.masked_graph(n, ranks, 0.30, 4)
    csr_rels = [(i, j, KC.known_entries_of(R, M), None) if M is not None else (i, j, R, None) for i, j, R, M in rels]
    Gc, Sc, Ec, _ = KC.run_plan(types, n, ranks, csr_rels, thetas, G0, dtype, 4)
    Gd, Sd, Ed, _ = KC.run_plan(types, n, ranks, rels, thetas, G0, dtype, 4)
    # (measured f64: G 1.7e-12)
    tol_g, tol_s, tol_e = {'f64': (5e-12, 1.2e-11, 3e-13), 'f32': (7e-6, 3.5e-5, 1.5e-7)}[dtype]
    for t in types:
        within(relerr(Gc[t], Gd[t]), tol_g, 'GPU %s forced lists vs dense completion, G_%s' % (dtype, t))
    for k in range(len(rels)):
        within(relerr(Sc[k], Sd[k]), tol_s, 'GPU %s forced lists vs dense completion, S_%d' % (dtype, k))
    within(np.max(np.abs(Ec - Ed) / Ed), tol_e, 'GPU %s forced lists vs dense completion, squared errors' % dtype)


def test_c5_golden_through_the_known_entries():
    from helpers import golden, movielens_style_graph, Snapshots, g0_from, compare_snapshots
    from skfusion_amd.fusion.decomposition import _dfmc
    z = golden('c5_movielens_scaled.npz')
    R, M, Theta, types, rank = movielens_style_graph()
    for key in R:
        if M[key][0] is not None:
            R[key] = [KC.known_entries_of(R[key][0], M[key][0])]
            M[key] = [None]
    snaps = Snapshots(range(6))
    _dfmc.dfmc(R, M, Theta, types, rank, max_iter=6, callback=snaps, G0=g0_from(z, 'dfmc/', types))
    assert compare_snapshots(z, 'dfmc/', snaps.snap, 1e-10) < 1e-10


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_api_list_path_equals_the_masked_array(dtype, monkeypatch, tmp_path):
    import known_csr_api_cases as A
    A.list_path_equals_mask_form(monkeypatch, 900, 700, 0.03, dtype, 10, tmp_path)


def test_api_stored_non_finite_values_take_the_fill(monkeypatch):
    import known_csr_api_cases as A
    A.nonfinite_with_constant_fill(monkeypatch, 600, 500, 'f64', 10)


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
def test_api_column_initialisers_from_the_entries(init_type, monkeypatch):
    import known_csr_api_cases as A
    A.column_initialisers(monkeypatch, 600, 500, init_type, 'f64', 10, 1e-7)      # (measured 2.1e-9)


@pytest.mark.parametrize('n_jobs', [1, 3])
def test_api_several_runs(n_jobs, monkeypatch):
    import known_csr_api_cases as A
    A.several_runs(monkeypatch, 600, 500, 'f64', 10, n_jobs)


def test_api_expanded_everywhere_else():
    import known_csr_api_cases as A
    A.expanded_cases(300, 250, 'f64', 10)


def _peak_rss_bytes():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024


def test_config5_shape_from_triplets_without_the_dense_form():
    """100k users x 40k movies, 80 M known ratings (2 %), bf16, rank 128: built from triplets, three iterations.  The
    mask form needs >= 36 GB on the host for this (f64 data + mask); here nothing of n_i x n_j is allocated anywhere."""
    import scipy.sparse
    from skfusion_amd.fusion.fusion_graph import Relation, ObjectType
    from skfusion_amd._engine import DevicePlan
    n_u, n_m, per_row = 100000, 40000, 800
    rss0 = _peak_rss_bytes()
    rs = np.random.RandomState(0)
    cols = rs.randint(0, n_m // per_row, (n_u, per_row), dtype=np.int32)
    cols += (np.arange(per_row, dtype=np.int32) * (n_m // per_row))[None, :]       # strictly ascending in every row
    vals = rs.randint(1, 11, n_u * per_row, dtype=np.int32).astype(np.float64)
    vals /= 10.0                                                                   # ratings 0.1 .. 1.0
    csr = scipy.sparse.csr_matrix((vals, cols.reshape(-1), np.arange(n_u + 1, dtype=np.int64) * per_row), shape=(n_u, n_m))
    del cols, vals
    users, movies = ObjectType('user', 128), ObjectType('movie', 128)
    ke = Relation(csr, users, movies, unstored='unknown').known_entries()
    del csr
    assert ke.known == n_u * per_row
    types, n, rank = ['user', 'movie'], {'user': n_u, 'movie': n_m}, {'user': 128, 'movie': 128}
    plan = DevicePlan(types, n, rank, [('user', 'movie', ke, None)], [], nat.SKF_DFMC, dtype='bf16')
    try:
        assert plan.workspace_bytes < 4 * 2 ** 30, plan.workspace_bytes
        G0 = {t: rs.rand(n[t], 128) * 0.1 + 0.01 for t in types}
        for t in types:
            plan.set_factor(t, G0[t])
        errs = []
        for _ in range(3):
            plan.iterate(1)
            errs.append(plan.relation_sqerr(0))
        G = {t: plan.get_factor(t) for t in types}
    finally:
        plan.close()
    for t in types:
        assert np.isfinite(G[t]).all()
    assert np.isfinite(errs).all() and errs[-1] < errs[0], errs
    grew = _peak_rss_bytes() - rss0
    assert grew < 4 * 2 ** 30, 'host peak RSS grew by %.2f GB' % (grew / 2 ** 30)
