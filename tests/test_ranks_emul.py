"""Ranks of held-out pairs (csrc/skf_complete.h, skf_complete_ranks, DeviceCompleter.ranks, FusionFit.complete_ranks) on the
host emulator: the small subset of tests/ranks_cases.py -- exact lattice cases index for index and bit for bit with P1
against the top-k operator, the random cases within their derived interval, NaN, every refusal, the public API."""
import ctypes as C
import os

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import ranks_cases as RC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


@pytest.mark.parametrize('ranks', [(5, 1), (5, 7), (64, 65)])
@pytest.mark.parametrize('n_cols', [7, 203])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_count_for_count_bit_for_bit(dtype, n_cols, ranks):
    RC.exact_case(dtype, 67, n_cols, ranks)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_two_row_tiles_and_many_column_tiles(dtype):
    RC.exact_case(dtype, 131, 997, (5, 7), patterns=('heavy',), splits=(0, 3, 32))


@pytest.mark.parametrize('pattern', ['none', 'edges', 'heavy'])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_random_within_the_derived_interval(dtype, pattern):
    RC.random_case(dtype, (20, 64), m=67, n_cols=203, pattern=pattern, label='emulator')


def test_bf16_name_scores_on_the_f32_masters():
    a = RC.random_case('f32', (20, 64), m=67, n_cols=203, pattern='none', label='emulator')
    b = RC.random_case('bf16', (20, 64), m=67, n_cols=203, pattern='none', label='emulator')
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_scores(dtype):
    RC.nan_case(dtype)


def test_refusals():
    RC.refusals_case('f64')
    RC.refusals_case('f32')


def test_refusals_need_no_device():
    """The product library (cross-compiled for gfx950), no device: these checks answer before any HIP call."""
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load_library()
    keep = (C.c_uint8 * 8192)()
    RC.refusals_without_device(lib, (C.addressof(keep) + 255) // 256 * 256)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, dtype, monkeypatch):
    RC.api_case(kind, dtype, monkeypatch)


def test_public_api_runs():
    RC.api_runs_case()
