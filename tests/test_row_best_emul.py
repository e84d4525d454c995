"""The k best columns of every row for any k (csrc/skf_complete.h complete_row_digits_kernel / complete_row_walk_kernel,
skf_complete_row_kth, DeviceCompleter.row_kth / row_best, FusionFit.complete_row_kth / complete_row_best) on the host emulator:
the small subset of tests/row_best_cases.py -- exact lattice cases index for index and bit for bit, P5 against top-k, P4 against
the above operator, the rank pass on random factors, NaN and infinities, independence of blocks and splits, the seam, every
refusal, guard bands, the public API."""
import ctypes as C
import os

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime
from guarded import guarded

import row_best_cases as RB


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


@pytest.mark.parametrize('ranks,signed', [((5, 1), False), ((5, 7), False), ((64, 65), False), ((5, 7), True)])
@pytest.mark.parametrize('n_cols', [7, 203])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_index_for_index_bit_for_bit(dtype, n_cols, ranks, signed):
    # (a select is five or ten walks and rank 64 costs the emulator twelve times rank 5: one exclusion pattern and two k there,
    # five k and one or two patterns elsewhere; every k, pattern and shape on the GPU)
    if ranks[0] == 64:
        few = {'patterns': ('heavy',), 'ks': (65, 'vector'), 'all_splits_at': ()}
    else:
        few = {'patterns': ('none', 'heavy') if (ranks, signed) == ((5, 7), False) else ('heavy',), 'ks': (1, 65, 100, n_cols + 5, 'vector')}
    trimmed = RB.exact_case(dtype, 67, n_cols, ranks, signed=signed, **few)
    assert trimmed > 0 or (ranks, n_cols) != ((5, 7), 203), 'no row has more pairs at its threshold than are wanted of them'


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_p5_ordered_is_topk(dtype):
    assert RB.p5_case(dtype, 67, 203, (5, 7), pattern='heavy') > 0           # (a row without candidates: the padding)
    RB.p5_case(dtype, 67, 7, (5, 1), pattern='none')


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_p4_above_at_the_thresholds(dtype):
    assert RB.p4_case(dtype, 67, 203, (5, 7), splits=(0, 3), cuts=(64,)) > 0    # (rows whose threshold is NaN occur)
    RB.p4_case(dtype, 67, 7, (5, 1), pattern='none', ks=(1, 9), splits=(1, 2), cuts=())


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_ranks_of_the_selected_pairs(dtype):
    RB.ranks_case(dtype)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_nan_and_infinities(dtype):
    RB.nan_inf_case(dtype)


def test_independent_of_blocks_splits_and_the_bf16_name():
    a = RB.independence_case('f32', m=67)
    assert RB.independence_case('bf16', m=67) == a, "the 'bf16' engine name must score on the f32 masters"


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exclusion_entries_on_either_side_of_a_split_boundary(dtype):
    RB.seam_case(dtype)


@pytest.mark.parametrize('which', ['range', 'descending', 'indptr'])
def test_invalid_exclusion_lists_are_refused_before_anything_is_counted(which):
    RB.refusal_order_case(which)


def test_refusals():
    RB.refusals_case('f64')
    RB.refusals_case('f32')
    RB.engine_refusals_case()


def test_refusals_need_no_device():
    """The product library (cross-compiled for gfx950), no device: these checks answer before any HIP call."""
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load_library()
    keep = (C.c_uint8 * 32768)()
    RB.refusals_without_device(lib, (C.addressof(keep) + 255) // 256 * 256)


def test_guard_bands():
    """The exact case and the refusals with guard bands around every buffer: no store outside the row histograms, the per-row
    words and the outputs at m = 67."""
    with guarded() as g:
        RB.exact_case('f32', 67, 203, (5, 7), patterns=('edges',), ks=(65, 'vector'))
        RB.refusals_case('f64')
    assert g.bands > 0


@pytest.mark.parametrize('kind', ['dfmc-masked', 'dfmf-csr'])
def test_public_api(kind, monkeypatch):
    RB.api_case(kind, monkeypatch)


def test_public_api_runs():
    RB.api_runs_case()
