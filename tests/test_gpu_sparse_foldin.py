"""Fold-ins through sparse relations given as their stored entries (SKF_REL_FOLD_CSR, skf_fold_lists) on the MI355X: the
operator bit for bit at every width class of fold_lists_kernel, whole fold-ins of every engine against the f64 host, the
error pass, every refused flag and list, the public API, and 200 000 new objects x 400 000 partners that are never expanded
anywhere (tests/sparse_foldin_cases.py)."""
import resource

import numpy as np
import pytest

import skfusion_amd._native as nat

import sparse_foldin_cases as FC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('c', [1, 5, 16, 63, 64, 65, 128, 200])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_fold_lists_bit_for_bit(dtype, c):
    for pattern in ('edges', 'full', 'heavy'):
        FC.fold_lists_case(131, 197, c, pattern, dtype)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_fold_lists_widest(dtype):
    FC.fold_lists_case(9, 197, 1024, 'full', dtype)


def test_fold_lists_refusals():
    FC.fold_lists_refusals()


RANKS = {'f64': (20, 64, 128), 'f32': (20, 64, 128), 'bf16': (64, 128, 256)}


@pytest.mark.parametrize('with_theta', [False, True])
@pytest.mark.parametrize('turn', [0, 1, 2])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_whole_fold_in_against_f64_host(dtype, turn, with_theta):
    """The three ranks of the engine, each in turn the target's (so that the pass runs at every width class)."""
    r = RANKS[dtype]
    ranks = {'t': r[turn], 'a': r[(turn + 1) % 3], 'b': r[(turn + 2) % 3]}
    FC.whole_case(dtype, ranks, with_theta, 'GPU %s ranks t/a/b %d/%d/%d theta %s' % (dtype, ranks['t'], ranks['a'], ranks['b'], with_theta))


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_all_zero_relation(dtype):
    r = RANKS[dtype]
    FC.zero_relation_case(dtype, {'t': r[1], 'a': r[0], 'b': r[2]}, 'GPU %s' % dtype)


def test_flag_combinations():
    FC.invalid_flag_cases()


@pytest.mark.parametrize('by_col', [False, True])
@pytest.mark.parametrize('kind', ['indptr', 'column', 'order', 'handover'])
def test_invalid_lists_are_refused_at_bind(kind, by_col):
    FC.invalid_lists_case(kind, 'bf16', by_col)


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_fold_lists_are_refused_before_any_gather(which):
    FC.refusal_order_case(which)


def test_api_formats_and_switches(monkeypatch):
    FC.api_formats_case('f64', ('csr', 'csc', 'coo'), monkeypatch)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_api_against_dense_yardstick(dtype, monkeypatch):
    FC.api_formats_case(dtype, ('csr',), monkeypatch, sizes=(300, 250, 40), ranks=(128, 64, 32), n_new=131)


def test_api_restarts_errors_initialiser_and_fill(monkeypatch):
    FC.api_runs_and_errors_case(monkeypatch)


def test_api_default_rule(monkeypatch):
    FC.api_rule_case(monkeypatch)


def _peak_rss_bytes():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024


def test_200k_new_objects_are_never_densified():
    """200 000 new objects x 400 000 partners, 40 entries each (8 M), bf16 plan, target rank 128 / partner rank 64, three
    iterations.  Derived, not measured: lists 8 M x 8 B + pointers ~ 0.07 GB; T = G_p S^T (400 000 x 128 f32, 0.2 GB), the
    partner's factor with its bf16 transpose (0.15 GB) and the target's n x c matrices G, Galt, E, D, Ec, Dc, H (~ 0.7 GB)
    ~ 1 GB -- workspace < 2 GiB (the dense f32 relation would be 320 GB); the host holds the lists (0.1 GB) and the
    factors: peak RSS growth < 1 GiB."""
    from skfusion_amd._engine import DevicePlan, KnownEntries
    n_t, n_p, per = 200000, 400000, 40
    rss0 = _peak_rss_bytes()
    rs = np.random.RandomState(0)
    step = n_p // per
    cols = rs.randint(0, step, (n_t, per), dtype=np.int32)
    cols += (np.arange(per, dtype=np.int32) * step)[None, :]                       # strictly ascending in every list
    vals = rs.randint(1, 64, n_t * per, dtype=np.int32).astype(np.float64)
    vals /= 8.0
    ke = KnownEntries(np.arange(n_t + 1, dtype=np.int64) * per, cols.reshape(-1), vals, (n_t, n_p), unstored='zero')
    del cols, vals
    types, n, rank = ['new', 'old'], {'new': n_t, 'old': n_p}, {'new': 128, 'old': 64}
    plan = DevicePlan(types, n, rank, [('new', 'old', ke, None)], [], nat.SKF_TRANSFORM, dtype='bf16', target='new')
    try:
        assert plan.workspace_bytes < 2 * 2 ** 30, plan.workspace_bytes
        plan.set_factor('old', (rs.rand(n_p, 64) * 0.1 + 0.01).astype(np.float32))
        plan.set_factor('new', (rs.rand(n_t, 128) * 0.1 + 0.01).astype(np.float32))
        plan.set_backbone(0, (rs.rand(128, 64) * 0.2).astype(np.float32))
        errs = []
        for _ in range(3):
            plan.iterate(1)
            errs.append(plan.relation_sqerr(0))
        finite = bool(np.isfinite(plan.get_factor('new')).all())
    finally:
        plan.close()
    assert finite
    assert np.isfinite(errs).all() and errs[2] <= errs[1] <= errs[0], errs
    grew = _peak_rss_bytes() - rss0
    assert grew < 2 ** 30, 'host peak RSS grew by %.2f GB' % (grew / 2 ** 30)
