"""Sparse constraints given as their entries (skf_theta_desc.data == NULL, skf_plan_set_constraint_entries) and the hub-row
split of the sparse constraint pass on the MI355X: entries-fed against dense-fed bit for bit in every engine and on every
schedule, the list path without a dense twin, hub rows cut into segments, every refusal, the public API, and a constraint
over 200 000 objects that is never expanded anywhere (tests/theta_csr_cases.py)."""
import resource

import numpy as np
import pytest

import skfusion_amd._native as nat

import theta_csr_cases as TC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('c', [20, 64])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_entries_equal_dense_small_graph_schedule(dtype, c, monkeypatch):
    TC.entries_against_dense('dfmf', dtype, c, monkeypatch, expect_small=True)


@pytest.mark.parametrize('c', [20, 64, 65, 130])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_entries_equal_dense_general_schedule(dtype, c, monkeypatch):
    """Each rank in turn the constrained type's: the 64-column sweep of the row walk and its tail.  Ranks up to 64 would
    ride the small-graph schedule in f64 / f32: forced off it."""
    TC.entries_against_dense('dfmf', dtype, c, monkeypatch, general=c <= 64, expect_small=False)


def test_entries_equal_dense_valu_engine(monkeypatch):
    TC.entries_against_dense('dfmf', 'f32', 65, monkeypatch, engine=nat.SKF_ENGINE_VALU)


@pytest.mark.parametrize('c', [20, 130])
@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_entries_equal_dense_dfmc(dtype, c, monkeypatch):
    TC.entries_against_dense('dfmc', dtype, c, monkeypatch)


@pytest.mark.parametrize('c', [20, 64, 65, 130])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_entries_equal_dense_fold_in(dtype, c, monkeypatch):
    TC.entries_against_dense('transform', dtype, c, monkeypatch)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_batched_restarts_share_the_entries(dtype):
    TC.batch_case(dtype)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_half_full_constraint_stays_lists(dtype):
    TC.half_full_case(dtype, 'GPU')


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_all_zero_constraint(dtype, monkeypatch):
    TC.all_zero_case(dtype, monkeypatch)


@pytest.mark.parametrize('c', [5, 64, 65, 130])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_hub_rows_split(dtype, c, monkeypatch):
    TC.hub_case(dtype, c, monkeypatch)


def test_hub_rows_on_both_sides_of_an_owner_boundary(monkeypatch):
    TC.hub_owned_case(monkeypatch)


@pytest.mark.parametrize('which', TC.BROKEN + ('handover', 'ok'))
def test_broken_lists_are_refused_at_bind_before_any_gather(which):
    TC.refusal_case(which, 'bf16' if which in ('range', 'order') else 'f64')


def test_setter_state_and_range():
    TC.setter_state_case()


def test_creation_checks():
    rt = nat.get_runtime()
    TC.creation_cases(rt.lib, rt.mem.empty(4096).ptr)


def test_api_constraint_entries(monkeypatch):
    TC.api_constraint_entries_case(monkeypatch)


@pytest.mark.parametrize('cls,dtype', [('Dfmf', 'f64'), ('Dfmf', 'f32'), ('Dfmf', 'bf16'), ('Dfmc', 'f64'), ('Dfmc', 'bf16')])
def test_api_fit_never_expands(cls, dtype, monkeypatch):
    TC.api_fit_case(cls, dtype, monkeypatch)


@pytest.mark.parametrize('dtype,n_run', [('f64', 1), ('f32', 2)])
def test_api_fold_in_never_expands(dtype, n_run, monkeypatch):
    TC.api_transform_case(dtype, monkeypatch, n_run=n_run)


def test_api_rule_and_switches(monkeypatch):
    TC.api_rule_case(monkeypatch)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_api_restarts_share_launches(dtype, monkeypatch):
    TC.api_restarts_case(dtype, monkeypatch)


def test_api_save_and_load(tmp_path, monkeypatch):
    TC.api_save_load_case(tmp_path, monkeypatch)


def _peak_rss_bytes():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024


def test_constraint_over_200k_objects_is_never_densified():
    """One type of 200 000 objects, rank 128, constrained by diagonal 0.02 + 8 entries of -0.001 per row (ascending strided
    buckets) + row 0 holding 100 000 entries of -1e-6 (a hub: 25 segments of 4096); one 200 000 x 50 000 sparse relation, 10
    entries a row, partner rank 64; bf16 engine, three iterations.  Derived, not measured: the constraint adds its lists
    (nnz x (4 + 4) B), pointers ((n + 1) x 8 B), the count scratch (n x 4 B) and the hub scratch (two partial matrices of
    (2 nnz / 4096 + 1) x 128 f32, the segment tables beside them inside the alignment allowance) -- the dense f32 form
    would be 160 GB; the host holds the lists and the factors: peak RSS growth < 1 GiB."""
    from skfusion_amd._engine import DevicePlan, KnownEntries
    n, n_p, per = 200000, 50000, 8
    rss0 = _peak_rss_bytes()
    rs = np.random.RandomState(0)
    width = n // per
    cols = rs.randint(0, width, (n, per)).astype(np.int64) + (np.arange(per, dtype=np.int64) * width)[None, :]
    own = np.arange(n, dtype=np.int64)[:, None]
    clash = cols == own                                             # (the diagonal is an entry of its own)
    cols[clash] += np.where(cols[clash] % width == width - 1, -1, 1)
    cols = np.concatenate([cols, own], axis=1)
    vals = np.concatenate([np.full((n, per), -0.001), np.full((n, 1), 0.02)], axis=1)
    order = np.argsort(cols, axis=1)
    cols, vals = np.take_along_axis(cols, order, axis=1), np.take_along_axis(vals, order, axis=1)
    hub_cols = np.concatenate([[0], np.arange(1, n, 2)])           # row 0: its diagonal + every odd column
    hub_vals = np.concatenate([[0.02], np.full(n // 2, -1e-6)])
    indices = np.concatenate([hub_cols, cols[1:].reshape(-1)]).astype(np.int32)
    values = np.concatenate([hub_vals, vals[1:].reshape(-1)])
    counts = np.full(n, per + 1, dtype=np.int64)
    counts[0] = hub_cols.size
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    theta = KnownEntries(indptr, indices, values, (n, n), unstored='zero')
    nnz = int(indices.size)
    del cols, vals, order, clash, own, indices, values
    step = n_p // 10
    rcols = rs.randint(0, step, (n, 10), dtype=np.int32) + (np.arange(10, dtype=np.int32) * step)[None, :]
    rel = KnownEntries(np.arange(n + 1, dtype=np.int64) * 10, rcols.reshape(-1), rs.randint(1, 9, n * 10) / 8.0, (n, n_p),
                       unstored='zero')
    del rcols
    types, nn, rank = ['obj', 'part'], {'obj': n, 'part': n_p}, {'obj': 128, 'part': 64}
    plain = DevicePlan(types, nn, rank, [('obj', 'part', rel, None)], [], nat.SKF_DFMF, dtype='bf16')
    ws_plain = plain.workspace_bytes
    plain.close()
    plan = DevicePlan(types, nn, rank, [('obj', 'part', rel, None)], [('obj', theta)], nat.SKF_DFMF, dtype='bf16')
    try:
        hub_scratch = 2 * (2 * nnz // 4096 + 1) * 128 * 4
        allowed = nnz * 8 + (n + 1) * 8 + n * 4 + hub_scratch + 2 ** 20
        assert plan.workspace_bytes - ws_plain <= allowed, (plan.workspace_bytes, ws_plain, allowed)
        for t in types:                 # (in place: no float64 temporaries of the factor's size beyond the draw itself)
            g0 = rs.rand(nn[t], rank[t]).astype(np.float32)
            g0 *= 0.1
            g0 += 0.01
            plan.set_factor(t, g0)
        del g0
        plan.iterate(3)
        G = {t: plan.get_factor(t) for t in types}
    finally:
        plan.close()
    for t in types:
        assert np.isfinite(G[t]).all() and (G[t] >= 0).all(), t
    grew = _peak_rss_bytes() - rss0
    assert grew < 2 ** 30, 'host peak RSS grew by %.2f GB' % (grew / 2 ** 30)
