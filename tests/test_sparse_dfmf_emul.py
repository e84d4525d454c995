"""Relations handed over as the CSR of their stored entries, zero elsewhere (SKF_REL_SPARSE_CSR), on the host emulator:
every valued list pass and the error pass against the host model, the lists a bind builds against scipy.sparse, invalid
lists and flag combinations, and whole fits against the dense-fed plan and the oracle (tests/sparse_dfmf_cases.py)."""
import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import sparse_dfmf_cases as SC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


# (rank of a = width of the Q gathers, rank of b = width of the P gathers) -> kernel variants of launch_srp
VARIANTS = [('f64', 16, 20), ('f64', 64, 32), ('f32', 32, 24), ('f32', 128, 64), ('bf16', 64, 128), ('bf16', 256, 20)]


@pytest.mark.parametrize('parts', [1, 2, 4, 8])
@pytest.mark.parametrize('dtype,rank_a,rank_b', VARIANTS)
def test_valued_passes_and_error_pass_against_host_model(dtype, rank_a, rank_b, parts, monkeypatch):
    pattern = ('edges', 'full', 'heavy')[(parts + rank_a) % 3]
    SC.pass_case(203, 197, rank_a, rank_b, dtype, parts, pattern,
                 'emulator %s ranks %d/%d parts %d %s' % (dtype, rank_a, rank_b, parts, pattern), monkeypatch, seed=parts)


@pytest.mark.parametrize('dtype,parts', [('f64', 1), ('f64', 8), ('f32', 2), ('bf16', 1), ('bf16', 4)])
def test_bound_lists_equal_scipy_lists(dtype, parts, monkeypatch):
    SC.lists_case(150, 130, 64, 24, dtype, parts, 0.06, monkeypatch, seed=parts)


@pytest.mark.parametrize('edits', [('empty',), ('full_row',), ('empty', 'full_row'), ('none',)])
def test_bound_lists_edge_patterns(edits, monkeypatch):
    SC.lists_case(259, 67, 20, 64, 'f32', 2, 0.05, monkeypatch, seed=3, edits=edits)


@pytest.mark.parametrize('kind', ['indptr', 'column', 'order', 'handover'])
@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_invalid_lists_are_refused_before_any_iteration(kind, dtype):
    SC.invalid_lists_case(kind, dtype)


def test_invalid_lists_are_refused_for_unmasked_dfmc_relations():
    SC.invalid_lists_case('order', 'f32', nat.SKF_DFMC)


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_stored_entries_are_refused_before_any_gather(which):
    SC.refusal_order_case(which)


def test_flag_combinations():
    SC.invalid_flag_cases()


N = {'a': 150, 'b': 130, 'c': 40}
TOL = {'f64': (1.5e-12, 6e-12, 1.3e-13), 'f32': (7e-6, 3.5e-5, 1.5e-7), 'bf16': (1.2e-2, 2.5e-2, 5.5e-4)}


@pytest.mark.parametrize('dtype,ranks', [('f64', {'a': 16, 'b': 12, 'c': 5}), ('f64', {'a': 70, 'b': 24, 'c': 66}),
                                         ('f32', {'a': 70, 'b': 24, 'c': 66}), ('bf16', {'a': 128, 'b': 64, 'c': 72})])
def test_csr_fed_fit_against_dense_fed_fit(dtype, ranks):
    SC.csr_against_dense(N, ranks, dtype, TOL[dtype], 'emulator %s' % dtype, density=(0.05, 0.03))


@pytest.mark.parametrize('kw', [dict(zero_rel=True), dict(empty_side=True)])
@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_all_zero_relation_and_empty_side(dtype, kw):
    ranks = {'a': 70, 'b': 24, 'c': 66} if dtype == 'f64' else {'a': 128, 'b': 64, 'c': 72}
    SC.csr_against_dense(N, ranks, dtype, TOL[dtype], 'emulator %s %s' % (dtype, sorted(kw)), density=(0.05, 0.03), **kw)


def test_csr_fed_dfmc_unmasked_relations():
    """Bounds: DFMC's list path against its dense path in f64 (tests/test_gpu_known_csr.py: G 5e-12, S 1.2e-11, error 3e-13)."""
    SC.csr_against_dense(N, {'a': 70, 'b': 24, 'c': 66}, 'f64', (5e-12, 1.2e-11, 3e-13), 'emulator DFMC', density=(0.05, 0.03),
                         variant=nat.SKF_DFMC)


def test_csr_fed_fit_against_oracle():
    SC.csr_against_oracle(N, {'a': 16, 'b': 12, 'c': 5}, 10, 1e-9, 'emulator', density=(0.05, 0.03))
    SC.csr_against_oracle(N, {'a': 70, 'b': 24, 'c': 66}, 10, 1e-9, 'emulator pipeline', density=(0.05, 0.03))
