"""Relations handed over as their known entries (SKF_REL_KNOWN_CSR) on the host emulator: the lists built from the CSR
on the device reproduce the mask form bit for bit, invalid lists end in SKF_E_INVALID before anything gathers through
them, and the public API routes scipy.sparse relations (Relation(..., unstored=...)) as documented."""
import numpy as np
import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import known_csr_cases as KC
from helpers import plan_create_status


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


N = {'a': 150, 'b': 130, 'c': 40}


@pytest.mark.parametrize('dtype,parts,rank_a', [('f64', 1, 64), ('f64', 8, 20), ('f32', 2, 64), ('f32', 1, 20),
                                               ('bf16', 1, 64), ('bf16', 2, 128), ('bf16', 8, 256)])
def test_csr_fed_lists_equal_mask_fed_lists(dtype, parts, rank_a, monkeypatch):
    KC.csr_against_mask(N, {'a': rank_a, 'b': 24, 'c': 5}, 0.06, dtype, parts, monkeypatch)


@pytest.mark.parametrize('edits', [('empty',), ('full_row',), ('empty', 'full_row'), ('none',)])
@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_csr_fed_edge_patterns(edits, dtype, monkeypatch):
    """Empty rows and columns, a fully known row, no known entry at all (nnz = 0)."""
    KC.csr_against_mask(N, {'a': 64, 'b': 24, 'c': 5}, 0.06, dtype, 2, monkeypatch, seed=3, edits=edits)


@pytest.mark.parametrize('dtype,parts', [('f64', 8), ('f32', 1), ('bf16', 2)])
def test_csr_fed_shapes_off_the_tile_multiples(dtype, parts, monkeypatch):
    """Object counts off the multiples of 4, 64 and 256."""
    KC.csr_against_mask({'a': 259, 'b': 67, 'c': 41}, {'a': 64, 'b': 24, 'c': 5}, 0.05, dtype, parts, monkeypatch, seed=1)


def _bad_plan(which):
    """A two-type DFMC plan whose only relation is handed over as a CSR that is not canonical."""
    from skfusion_amd._engine import DevicePlan, DeviceKnownEntries
    rs = np.random.RandomState(0)
    indptr = np.array([0, 2, 4, 4, 6], dtype=np.int64)
    idx = np.array([1, 3, 0, 2, 4, 5], dtype=np.int32)
    if which == 'range':
        idx[3] = 6                                      # column 6 of 6
    elif which == 'descending':
        idx[2], idx[3] = 2, 0
    elif which == 'indptr':
        indptr[2] = 1                                   # 2 -> 1 -> 4: a negative step
    vals = rs.rand(6)
    mem = nat.get_runtime().mem
    dev = DeviceKnownEntries(mem.from_host(indptr), mem.from_host(idx), mem.from_host(vals), (4, 6), 6)
    return lambda: DevicePlan(['a', 'b'], {'a': 4, 'b': 6}, {'a': 2, 'b': 2}, [('a', 'b', dev, None)], [], nat.SKF_DFMC)


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_lists_are_refused_before_any_gather(which):
    from skfusion_amd._engine import launch_count
    make = _bad_plan(which)
    before = launch_count()
    with pytest.raises(nat.SkfNativeError) as err:
        make()
    assert err.value.code == nat.SKF_E_INVALID
    assert launch_count() - before == 1                 # the validation kernel, nothing after it
    plan = _bad_plan('ok')()                            # (the same plan with canonical lists binds)
    plan.close()


def test_known_csr_flag_is_refused_where_it_does_not_apply():
    """The flag on DFMF / fold-in plans, on row blocks, and a missing skf_plan_set_known_entries."""
    import ctypes as C
    rt = nat.get_runtime()
    t = (nat.TypeDesc * 2)()
    t[0].n_obj, t[0].rank, t[1].n_obj, t[1].rank = 4, 2, 6, 2
    r = (nat.RelationDesc * 1)()
    r[0].row_type, r[0].col_type, r[0].flags, r[0].known_bound = 0, 1, nat.SKF_REL_KNOWN_CSR, 3
    sizes, known_csr = [(4, 2), (6, 2)], dict(row_type=0, col_type=1, flags=nat.SKF_REL_KNOWN_CSR, known_bound=3)
    for variant in (nat.SKF_DFMF, nat.SKF_TRANSFORM):
        assert plan_create_status(rt.lib, sizes, [known_csr], variant=variant, target=0)[0] == nat.SKF_E_INVALID
    assert plan_create_status(rt.lib, sizes, [dict(known_csr, n_rows=2)], variant=nat.SKF_DFMC)[0] == nat.SKF_E_INVALID      # a row block
    h = nat._P()
    rt.call('skf_plan_create', 2, t, 1, r, 0, None, C.byref(nat.Options(nat.SKF_F64, nat.SKF_DFMC, -1, 0, 0, 0, 0)),
            C.byref(h))
    try:
        nbytes = C.c_size_t()
        rt.call('skf_plan_workspace_bytes', h, C.byref(nbytes))
        ws = rt.mem.empty(nbytes.value)
        assert rt.lib.skf_plan_bind_workspace(h, ws.ptr, nbytes.value, None) == nat.SKF_E_INVALID
    finally:
        rt.call('skf_plan_destroy', h)


def test_host_validation_mirrors_the_device_checks():
    from skfusion_amd._engine import KnownEntries
    from skfusion_amd.fusion.base import DataFusionError
    ok = KnownEntries([0, 2, 2, 3], [0, 4, 1], [1., 2., 3.], (3, 5))
    ok.validate()
    for bad in (KnownEntries([0, 2, 2, 3], [0, 5, 1], [1., 2., 3.], (3, 5)),       # index out of range
                KnownEntries([0, 2, 2, 3], [4, 0, 1], [1., 2., 3.], (3, 5)),       # descending
                KnownEntries([0, 2, 1, 3], [0, 4, 1], [1., 2., 3.], (3, 5)),       # non-monotone indptr
                KnownEntries([0, 2, 2, 3], [0, 0, 1], [1., 2., 3.], (3, 5)),       # a duplicate
                KnownEntries([0, 2, 2, 2], [0, 4, 1], [1., 2., 3.], (3, 5))):      # indptr does not end at nnz
        with pytest.raises(DataFusionError):
            bad.validate()


# ---- the public API (small sizes; the GPU repeats them larger: tests/test_gpu_known_csr.py) ---------------------------
def test_api_list_path_equals_the_masked_array(monkeypatch, tmp_path):
    import known_csr_api_cases as A
    A.list_path_equals_mask_form(monkeypatch, 70, 90, 0.05, 'f64', 3, tmp_path)
    A.list_path_equals_mask_form(monkeypatch, 70, 90, 0.05, 'bf16', 2)


def test_api_stored_non_finite_values_take_the_fill(monkeypatch):
    import known_csr_api_cases as A
    A.nonfinite_with_constant_fill(monkeypatch, 60, 50, 'f64', 2)


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
def test_api_column_initialisers_from_the_entries(init_type, monkeypatch):
    import known_csr_api_cases as A
    A.column_initialisers(monkeypatch, 60, 50, init_type, 'f64', 2, 1e-9)


@pytest.mark.parametrize('n_jobs', [1, 3])
def test_api_several_runs(n_jobs, monkeypatch):
    """(n_jobs = 3: the restarts share one upload of the graph, upload_graph)"""
    import known_csr_api_cases as A
    A.several_runs(monkeypatch, 60, 50, 'f64', 2, n_jobs)


def test_api_expanded_everywhere_else():
    import known_csr_api_cases as A
    A.expanded_cases(40, 30, 'f64', 2)


def test_relation_keyword_and_dense_form():
    import scipy.sparse
    from skfusion_amd.fusion import Relation, ObjectType
    a, b = ObjectType('a', 2), ObjectType('b', 2)
    with pytest.raises(ValueError):
        Relation(np.zeros((2, 2)), a, b, unstored='nothing')
    coo = scipy.sparse.coo_matrix(([1.0, 2.0, 0.0, 5.0], ([0, 0, 1, 0], [1, 1, 0, 2])), shape=(2, 3))
    r = Relation(coo, a, b, unstored='unknown')
    ke = r.known_entries()
    assert list(ke.indptr) == [0, 2, 3] and list(ke.indices) == [1, 2, 0] and list(ke.values) == [3.0, 5.0, 0.0]
    d = r.dense_data()
    assert d.mask.tolist() == [[True, False, False], [False, True, True]]
    assert np.array_equal(Relation(coo, a, b).dense_data(), coo.toarray())
    assert coo.nnz == 4                                 # the caller's matrix is left as it was


def test_c5_golden_through_the_known_entries(monkeypatch):
    """The scaled config 5 with the ratings handed over as KnownEntries reproduces the reference golden (functional seam)."""
    import known_csr_cases as KC
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
