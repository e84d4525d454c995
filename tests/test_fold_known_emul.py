"""Fold-ins on the known entries only (SKF_REL_FOLD_CSR | SKF_REL_FOLD_KNOWN, skf_fold_known_pass, fusion.DfmcTransform) on
the host emulator: the operator bit for bit, whole fold-ins against the f64 host model, the properties, the planted data,
every refusal (tests/fold_known_cases.py)."""
import ctypes as C
import os

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import fold_known_cases as FK


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


@pytest.mark.parametrize('with_x', [True, False])
@pytest.mark.parametrize('c', [1, 5, 64, 65, 130])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_fold_known_pass_bit_for_bit(dtype, c, with_x):
    for pattern in ('edges', 'full', 'heavy'):
        FK.pass_case(37, 41, c, pattern, dtype, with_x)


def test_fold_known_pass_refusals():
    FK.pass_refusals()


N = {'t': 37, 'a': 41, 'b': 30}


@pytest.mark.parametrize('with_theta', [False, True])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('ranks', [{'t': 8, 'a': 20, 'b': 8}, {'t': 20, 'a': 8, 'b': 20}])
def test_whole_fold_in_against_f64_host_model(dtype, ranks, with_theta):
    FK.whole_case(dtype, ranks, with_theta, 'emulator %s c_t %d theta %s' % (dtype, ranks['t'], with_theta), n=N)


def test_whole_fold_in_bf16_plan_and_a_wide_target():
    FK.whole_case('bf16', {'t': 70, 'a': 8, 'b': 20}, False, 'emulator bf16 c_t 70', n=N)


def test_every_entry_known_is_the_plain_fold_in():
    FK.all_known_case('f64', {'t': 20, 'a': 8, 'b': 8}, 'emulator f64', n=N)


def test_known_entry_error_does_not_increase():
    FK.monotone_case('f64', {'t': 8, 'a': 20, 'b': 8}, 'emulator f64', n=N)


def test_flag_combinations():
    FK.invalid_flag_cases()


@pytest.mark.parametrize('by_col', [False, True])
@pytest.mark.parametrize('kind', ['indptr', 'column', 'order', 'handover'])
def test_invalid_lists_are_refused_at_bind(kind, by_col):
    FK.invalid_lists_case(kind, 'f64', by_col)


def test_creation_checks_need_no_device():
    """The product library (cross-compiled for gfx950), no device: the plan-creation checks answer before any HIP call."""
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load_library()
    FK.creation_flag_cases(lib)


def test_api_formats_masked_arrays_and_host_model(monkeypatch):
    FK.api_formats_case('f64', ('csr', 'csc', 'coo'), monkeypatch)


def test_api_f32(monkeypatch):
    FK.api_formats_case('f32', ('csr', 'coo'), monkeypatch)


def test_api_without_unknown_cells_is_dfmf_transform(monkeypatch):
    FK.api_no_unknown_case(monkeypatch)


def test_api_restarts_stopping_fill_and_preprocessor():
    FK.api_restarts_stopping_and_fill_case()


@pytest.mark.parametrize('known_share', [0.1, 0.3])
def test_planted_data_held_out_rmse(known_share):
    FK.planted_case(known_share)
