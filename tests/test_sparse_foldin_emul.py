"""Fold-ins through sparse relations given as their stored entries (SKF_REL_FOLD_CSR, skf_fold_lists) on the host emulator:
the operator bit for bit, whole fold-ins against the f64 host, the error pass, every refused flag and list, and the public
API (tests/sparse_foldin_cases.py)."""
import ctypes as C
import os

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import sparse_foldin_cases as FC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


@pytest.mark.parametrize('c', [5, 64, 65])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_fold_lists_bit_for_bit(dtype, c):
    for pattern in ('edges', 'full', 'heavy'):
        FC.fold_lists_case(37, 41, c, pattern, dtype)


def test_fold_lists_refusals():
    FC.fold_lists_refusals()


N = {'t': 37, 'a': 41, 'b': 30}


@pytest.mark.parametrize('with_theta', [False, True])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('ranks', [{'t': 8, 'a': 20, 'b': 8}, {'t': 20, 'a': 8, 'b': 20}])
def test_whole_fold_in_against_f64_host(dtype, ranks, with_theta):
    FC.whole_case(dtype, ranks, with_theta, 'emulator %s c_t %d theta %s' % (dtype, ranks['t'], with_theta), n=N)


def test_wide_target_rank_takes_the_swept_kernel():
    FC.whole_case('f32', {'t': 70, 'a': 8, 'b': 20}, False, 'emulator f32 c_t 70', n=N)


@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_all_zero_relation(dtype):
    FC.zero_relation_case(dtype, {'t': 20, 'a': 8, 'b': 8}, 'emulator %s' % dtype, n=N)


def test_flag_combinations():
    FC.invalid_flag_cases()


@pytest.mark.parametrize('by_col', [False, True])
@pytest.mark.parametrize('kind', ['indptr', 'column', 'order', 'handover'])
def test_invalid_lists_are_refused_at_bind(kind, by_col):
    FC.invalid_lists_case(kind, 'f64', by_col)


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_fold_lists_are_refused_before_any_gather(which):
    FC.refusal_order_case(which)


def test_creation_checks_need_no_device():
    """The product library (cross-compiled for gfx950), no device: the plan-creation checks answer before any HIP call."""
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load_library()
    keep = (C.c_uint8 * 4096)()
    FC.creation_flag_cases(lib, C.addressof(keep))
    assert FC.create_status(lib, nat.SKF_DFMF, nat.SKF_REL_FOLD_CSR) == nat.SKF_E_INVALID
    assert b'SKF_REL_FOLD_CSR' in lib.skf_last_error()


def test_api_formats_and_switches(monkeypatch):
    FC.api_formats_case('f64', ('csr', 'csc', 'coo'), monkeypatch)


def test_api_f32_against_dense_yardstick(monkeypatch):
    FC.api_formats_case('f32', ('csr',), monkeypatch)


def test_api_restarts_errors_initialiser_and_fill(monkeypatch):
    FC.api_runs_and_errors_case(monkeypatch)


def test_api_default_rule(monkeypatch):
    FC.api_rule_case(monkeypatch)
