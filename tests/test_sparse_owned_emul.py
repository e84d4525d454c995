"""CSR-fed relations under row ownership (SKF_OPT_OWNED_ROWS, `shard='owned'`) on the host emulator: plan creation, the
lists a bind builds from a row slice, invalid slices, f64 fits against the oracle, every engine against the dense-fed owned
fit with the exchange accounting, the never-expanded conditions and early stopping (tests/sparse_owned_cases.py).  The ranks
of a group are threads of this process (helpers.ThreadGroup)."""
import pytest

from emul.runtime import emulated_runtime, use_runtime

import sparse_owned_cases as OC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


def test_creation_of_csr_fed_relations_on_owned_plans():
    OC.creation_cases()


def test_an_absent_relation_takes_no_lists():
    OC.absent_handover_case()


@pytest.mark.parametrize('unstored', ['zero', 'unknown'])
@pytest.mark.parametrize('dtype,size,parts', [('f64', 2, 1), ('f64', 3, 4), ('f32', 2, 4), ('f32', 3, 1), ('bf16', 2, 4), ('bf16', 3, 1)])
def test_bound_lists_of_every_rank_equal_scipy_lists_of_its_slice(dtype, size, parts, unstored, monkeypatch):
    OC.lists_case(dtype, size, parts, unstored, monkeypatch, seed=size + parts)


@pytest.mark.parametrize('unstored', ['zero', 'unknown'])
def test_bound_lists_with_a_rank_that_owns_no_row(unstored, monkeypatch):
    OC.lists_case('bf16', 3, 4, unstored, monkeypatch, seed=5, n_a=120)


@pytest.mark.parametrize('unstored', ['zero', 'unknown'])
@pytest.mark.parametrize('which', ['offset', 'range', 'descending'])
def test_invalid_slices_are_refused_before_any_gather(which, unstored):
    OC.invalid_slice_case(which, unstored)


# (the emulator runs a subset of the GPU module's cases -- every engine, both worlds, an absent rank --: the bf16 ranks
# 256 / 128 / 64 take minutes on it)
F64 = [({'a': 16, 'b': 12, 'c': 8}, 2, 1), ({'a': 16, 'b': 12, 'c': 8}, 3, 4),
       ({'a': 70, 'b': 128, 'c': 33}, 2, 4), ({'a': 70, 'b': 128, 'c': 33}, 3, 1)]


@pytest.mark.parametrize('ranks,size,parts', F64)
def test_csr_fed_owned_dfmf_against_the_oracle(ranks, size, parts, monkeypatch):
    OC.dfmf_against_oracle(ranks, size, parts, monkeypatch)


@pytest.mark.parametrize('ranks,size,parts', F64)
def test_csr_fed_owned_dfmc_against_the_oracle(ranks, size, parts, monkeypatch):
    OC.dfmc_against_oracle(ranks, size, parts, monkeypatch)


@pytest.mark.parametrize('key,size,parts', [('f64-narrow', 2, 4), ('f64-wide', 3, 4), ('f32', 2, 1), ('bf16-128', 3, 4)])
def test_csr_fed_owned_dfmf_against_dense_fed_owned_dfmf(key, size, parts, monkeypatch):
    OC.dfmf_csr_against_dense(key, size, parts, monkeypatch)


@pytest.mark.parametrize('key,size,parts', [('f64-narrow', 3, 1), ('f32', 2, 1), ('bf16-128', 3, 4)])
def test_csr_fed_owned_dfmc_against_mask_fed_owned_dfmc(key, size, parts, monkeypatch):
    OC.dfmc_csr_against_dense(key, size, parts, monkeypatch)


def test_owned_plans_never_expand_their_slices(monkeypatch):
    OC.never_expanded_plans(monkeypatch, iterate=False)         # (the iterations at this size: tests/test_gpu_sparse_owned.py)


def test_api_owned_fits_never_expand_the_relation(monkeypatch):
    from skfusion_amd.fusion import Dfmf, Dfmc
    OC.never_expanded_api(Dfmf, monkeypatch)
    OC.never_expanded_api(Dfmc, monkeypatch)
    OC.never_expanded_api(Dfmc, monkeypatch, wide=True)


def test_stopping_system_on_a_csr_fed_owned_fit():
    OC.stopping_case()
