"""Fold-ins on the known entries only (SKF_REL_FOLD_CSR | SKF_REL_FOLD_KNOWN, skf_fold_known_pass, fusion.DfmcTransform) on
the MI355X: the operator bit for bit at every width class of fold_known_kernel, whole fold-ins of every engine against the
f64 host model, the properties, the planted data, every refusal, and 200 000 new objects x 400 000 partners that are never
expanded anywhere (tests/fold_known_cases.py)."""
import resource

import numpy as np
import pytest

import skfusion_amd._native as nat

import fold_known_cases as FK

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('with_x', [True, False])
@pytest.mark.parametrize('c', [1, 5, 16, 63, 64, 65, 128, 200])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_fold_known_pass_bit_for_bit(dtype, c, with_x):
    for pattern in ('edges', 'full', 'heavy'):
        FK.pass_case(131, 197, c, pattern, dtype, with_x)


@pytest.mark.parametrize('with_x', [True, False])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_fold_known_pass_widest(dtype, with_x):
    FK.pass_case(9, 197, 1024, 'full', dtype, with_x)


def test_fold_known_pass_refusals():
    FK.pass_refusals()


RANKS = {'f64': (20, 64, 128), 'f32': (20, 64, 128), 'bf16': (64, 128, 256)}


@pytest.mark.parametrize('with_theta', [False, True])
@pytest.mark.parametrize('turn', [0, 1, 2])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_whole_fold_in_against_f64_host_model(dtype, turn, with_theta):
    """The three ranks of the engine, each in turn the target's (so that the pass runs at every width class).

    f32 / bf16: the masked plan's deviation from its f64 host model against 4 x the deviation of the dense-fed plan of the
    same engine on the zero-filled relations from oracle.dfmf_oracle.transform (tests/fold_known_cases.py, item 2)."""
    r = RANKS[dtype]
    ranks = {'t': r[turn], 'a': r[(turn + 1) % 3], 'b': r[(turn + 2) % 3]}
    FK.whole_case(dtype, ranks, with_theta, 'GPU %s ranks t/a/b %d/%d/%d theta %s' % (dtype, ranks['t'], ranks['a'], ranks['b'], with_theta))


def test_every_entry_known_is_the_plain_fold_in():
    FK.all_known_case('f64', {'t': 64, 'a': 20, 'b': 128}, 'GPU f64')


def test_known_entry_error_does_not_increase():
    FK.monotone_case('f64', {'t': 20, 'a': 64, 'b': 128}, 'GPU f64')


def test_flag_combinations():
    FK.invalid_flag_cases()


@pytest.mark.parametrize('by_col', [False, True])
@pytest.mark.parametrize('kind', ['indptr', 'column', 'order', 'handover'])
def test_invalid_lists_are_refused_at_bind(kind, by_col):
    FK.invalid_lists_case(kind, 'bf16', by_col)


def test_api_formats_masked_arrays_and_host_model(monkeypatch):
    FK.api_formats_case('f64', ('csr', 'csc', 'coo'), monkeypatch)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_api_f32_and_bf16(dtype, monkeypatch):
    FK.api_formats_case(dtype, ('csr', 'coo'), monkeypatch, sizes=(300, 250, 40), ranks=(128, 64, 32), n_new=131)


def test_api_without_unknown_cells_is_dfmf_transform(monkeypatch):
    FK.api_no_unknown_case(monkeypatch)


def test_api_restarts_stopping_fill_and_preprocessor():
    FK.api_restarts_stopping_and_fill_case()


@pytest.mark.parametrize('known_share', [0.1, 0.3])
def test_planted_data_held_out_rmse(known_share):
    FK.planted_case(known_share)


def _peak_rss_bytes():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024


def test_200k_new_objects_are_never_densified():
    """200 000 new objects x 400 000 partners, 40 known entries each (8 M), bf16 plan, target rank 128 / partner rank 64,
    three iterations.  Derived, not measured (the arithmetic of the stored-entry fold-in's test of this shape): lists 8 M x 8 B
    + pointers ~ 0.07 GB; T = G_p S^T (400 000 x 128 f32, 0.2 GB), the partner's factor with its bf16 transpose (0.15 GB)
    and the target's n x c matrices G, Galt, E, D, Ec, Dc and -- in place of H -- the one n_t x c scratch X (~ 0.7 GB)
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
    ke = KnownEntries(np.arange(n_t + 1, dtype=np.int64) * per, cols.reshape(-1), vals, (n_t, n_p), unstored='unknown')
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
