"""Scores at or above a threshold as CSR (csrc/skf_complete.h, skf_complete_above, DeviceCompleter.above,
FusionFit.complete_above) on the host emulator: the small subset of tests/above_cases.py -- exact lattice cases index for
index and bit for bit, P2 against the top-k operator and the agreement with the rank operator, the random cases under their
derived bound, NaN, every refusal, the public API."""
import ctypes as C
import os

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import above_cases as AC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


@pytest.mark.parametrize('ranks', [(5, 1), (5, 7), (64, 65)])
@pytest.mark.parametrize('n_cols', [7, 203])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_index_for_index_bit_for_bit(dtype, n_cols, ranks):
    AC.exact_case(dtype, 67, n_cols, ranks)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_three_row_tiles_and_many_column_tiles(dtype):
    AC.exact_case(dtype, 131, 997, (5, 7), patterns=('heavy',), splits=(0, 3, 32))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exclusion_entries_on_either_side_of_a_split_boundary(dtype):
    AC.seam_case(dtype)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_scan_over_several_chunks_of_rows(dtype):
    AC.scan_case(dtype, 600)


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_exclusion_lists_are_refused_before_any_gather(which):
    AC.refusal_order_case(which)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_agrees_with_topk_and_ranks(dtype):
    assert AC.agreement_case(dtype, 67, 203, (5, 7)) > 0             # rank 5: ties beyond the k-th entry exist
    AC.agreement_case(dtype, 67, 7, (5, 1), pattern='none')
    AC.agreement_case(dtype, 67, 203, (20, 64), pattern='heavy', factors=AC.random_factors)


@pytest.mark.parametrize('pattern', ['none', 'edges', 'heavy'])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_random_under_the_derived_bound(dtype, pattern):
    AC.random_case(dtype, (20, 64), m=67, n_cols=203, pattern=pattern, label='emulator')


def test_bf16_name_scores_on_the_f32_masters():
    a = AC.random_case('f32', (20, 64), m=67, n_cols=203, pattern='none', label='emulator')
    b = AC.random_case('bf16', (20, 64), m=67, n_cols=203, pattern='none', label='emulator')
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_scores(dtype):
    AC.nan_case(dtype)


def test_refusals():
    AC.refusals_case('f64')
    AC.refusals_case('f32')


def test_refusals_need_no_device():
    """The product library (cross-compiled for gfx950), no device: these checks answer before any HIP call."""
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load_library()
    keep = (C.c_uint8 * 32768)()
    AC.refusals_without_device(lib, (C.addressof(keep) + 255) // 256 * 256)


@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, monkeypatch):
    AC.api_case(kind, monkeypatch)


def test_public_api_runs():
    AC.api_runs_case()
