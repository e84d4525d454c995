"""Score histograms and ROC / PR curves (csrc/skf_complete.h complete_hist_kernel, skf_complete_hist, DeviceCompleter.hist /
histogram, FusionFit.complete_histogram / complete_curve) on the host emulator: the small subset of tests/hist_cases.py --
exact lattice cases bin for bin, more than 2047 edges in walks, P6 against the above operator and P7 against the rank pass,
the random cases under their derived bound, NaN and infinities, independence of the blocks and splits, every refusal, guard
bands, the public API and the curve."""
import ctypes as C
import os

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime
from guarded import guarded

import hist_cases as HC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


@pytest.mark.parametrize('ranks,signed', [((5, 1), False), ((5, 7), False), ((64, 65), False), ((5, 7), True)])
@pytest.mark.parametrize('n_cols', [7, 203])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_bin_for_bin(dtype, n_cols, ranks, signed):
    # (rank 64 costs the emulator twelve times rank 5: one exclusion pattern and two split counts there, all on the GPU)
    HC.exact_case(dtype, 67, n_cols, ranks, signed=signed, **({'patterns': ('heavy',), 'splits': (0, 1, 2, 3)} if ranks[0] == 64 else {}))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_more_than_2047_edges_take_several_walks(dtype):
    HC.walks_case(dtype, 67, 203, n_distinct=2708)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_p6_the_bins_above_an_edge_are_above_at_that_threshold(dtype):
    HC.p6_case(dtype, 67, 203, (5, 7))
    HC.p6_case(dtype, 67, 7, (5, 1), pattern='none', split_pairs=((0, 3),))
    HC.p6_case(dtype, 67, 203, (5, 7), pattern='heavy', split_pairs=((1, 2),), signed=True)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_p7_a_target_lands_in_the_bin_of_its_rank_score(dtype):
    HC.p7_case(dtype, 67, 203, (5, 7))
    HC.p7_case(dtype, 67, 203, (5, 7), pattern='heavy', signed=True)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_random_under_the_derived_bound(dtype):
    HC.random_case(dtype, (20, 64), m=67, n_cols=203, label='emulator')


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_and_infinities(dtype):
    HC.nan_inf_case(dtype)


def test_independent_of_blocks_splits_and_the_bf16_name():
    a = HC.independence_case('f32')
    assert HC.independence_case('bf16') == a, "the 'bf16' engine name must score on the f32 masters"


def test_refusals():
    HC.refusals_case('f64')
    HC.refusals_case('f32')


def test_refusals_need_no_device():
    """The product library (cross-compiled for gfx950), no device: these checks answer before any HIP call."""
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load_library()
    keep = (C.c_uint8 * 32768)()
    HC.refusals_without_device(lib, (C.addressof(keep) + 255) // 256 * 256)


def test_refusals_of_the_python_layers():
    HC.python_refusals_case()


def test_between_guard_bands():
    with guarded():
        HC.exact_case('f32', 67, 203, (5, 7), patterns=('heavy',), splits=(0, 3))
    with guarded():
        HC.refusals_case('f32')


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_curve_counts_and_mid_rank_auroc_exactly(dtype):
    HC.curve_case(dtype)
    HC.curve_case(dtype, n_cols=7, ranks=(5, 1), pattern='none')
    HC.curve_case(dtype, pattern='heavy', signed=True)


def test_default_edges_bound_the_float64_auroc():
    HC.default_edges_case()


@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, monkeypatch):
    HC.api_case(kind, monkeypatch)


def test_public_api_runs():
    HC.api_runs_case()
