"""The n best pairs of a whole relation (csrc/skf_complete.h complete_digits_kernel, skf_complete_digits,
DeviceCompleter.digits / kth, FusionFit.complete_kth / complete_best) on the host emulator: the small subset of
tests/best_cases.py -- exact lattice cases index for index and bit for bit, the raw histograms against the host's keys,
P3 against the above operator, a single row against top-k, the random cases under their derived bound, NaN and
infinities, independence of the blocks and splits, every refusal, the public API."""
import ctypes as C
import os

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import best_cases as BC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


def test_digit_walk_is_a_pure_function_of_the_histograms():
    BC.digit_walk_case()


@pytest.mark.parametrize('ranks,signed', [((5, 1), False), ((5, 7), False), ((64, 65), False), ((5, 7), True)])
@pytest.mark.parametrize('n_cols', [7, 203])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_index_for_index_bit_for_bit(dtype, n_cols, ranks, signed):
    # (rank 64 costs the emulator twelve times rank 5: one exclusion pattern there, all three on the GPU)
    ties = BC.exact_case(dtype, 67, n_cols, ranks, signed=signed, **({'patterns': ('heavy',)} if ranks[0] == 64 else {}))
    assert ties > 0 or ranks != (5, 1), 'no tie class larger than what is wanted of it is exercised'


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exclusion_entries_on_either_side_of_a_split_boundary(dtype):
    BC.seam_case(dtype)


@pytest.mark.parametrize('signed', [False, True])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_every_pass_is_the_bincount_of_the_host_keys(dtype, signed):
    BC.digits_case(dtype, 67, 203, (5, 7), signed=signed)
    BC.digits_case(dtype, 67, 7, (5, 1), signed=signed, pattern='none', splits=(0, 2))


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_exclusion_lists_are_refused_before_anything_is_counted(which):
    BC.refusal_order_case(which)


def test_refusals():
    BC.refusals_case('f64')
    BC.refusals_case('f32')


def test_refusals_need_no_device():
    """The product library (cross-compiled for gfx950), no device: these checks answer before any HIP call."""
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load_library()
    keep = (C.c_uint8 * 32768)()
    BC.refusals_without_device(lib, (C.addressof(keep) + 255) // 256 * 256)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_p3_and_agreement_with_above_and_ranks(dtype):
    assert BC.agreement_case(dtype, 67, 203, (5, 7)) > 0              # rank 5: ties at the n-th score exist
    BC.agreement_case(dtype, 67, 7, (5, 1), pattern='none', ns=(1, 64))
    BC.agreement_case(dtype, 67, 203, (20, 64), pattern='heavy', factors=BC.random_factors, ns=(300,))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_single_row_is_topk(dtype):
    BC.single_row_case(dtype, 203, (5, 7))
    BC.single_row_case(dtype, 7, (5, 1), pattern='none')


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_random_under_the_derived_bound(dtype):
    BC.random_case(dtype, (20, 64), m=67, n_cols=203, n=300, label='emulator')


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_and_infinities(dtype):
    BC.nan_inf_case(dtype)


def test_independent_of_blocks_splits_and_the_bf16_name():
    a = BC.independence_case('f32')
    assert BC.independence_case('bf16') == a, "the 'bf16' engine name must score on the f32 masters"


@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, monkeypatch):
    BC.api_case(kind, monkeypatch)


def test_public_api_runs():
    BC.api_runs_case()
