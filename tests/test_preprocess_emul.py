"""The operators that touch a relation before the engine does -- skf_fill_unknown, skf_cast, skf_to_bf16, skf_fill_uniform
(tests/preprocess_cases.py) -- on the host emulator, through the C ABI, between guard bands: the float64 model of the fill
held to the reference's recorded outputs, then the kernels held to the model bit for bit at every shape of SEAMS; the casts
against NumPy's; the bf16 conversion and nat.to_bf16_bits against an independent statement of round-to-nearest-even on every
bf16 pattern; every refusal.  The emulator runs the large shapes of SEAMS too where a case stays under about ten seconds
(profiles/preprocess_ops.txt has the times); the structure cases at 8209 x 67 and the 2 097 185-row conversion are GPU-only."""
import time

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import preprocess_cases as PC

F64, F32, BF16 = nat.SKF_F64, nat.SKF_F32, nat.SKF_BF16
TIMES = []


@pytest.fixture(scope='module', autouse=True)
def emul():
    with use_runtime(emulated_runtime()) as rt:
        yield rt


@pytest.fixture(autouse=True)
def timed(request):
    t0 = time.time()
    yield
    TIMES.append((time.time() - t0, request.node.name))


def test_the_model_is_the_reference():
    assert PC.model_against_golden() > 800


@pytest.mark.parametrize('kind', PC.KINDS)
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', PC.SEAMS, ids=PC.shape_id)
def test_fill_exact_data_byte_for_byte(shape, dtype, kind):
    PC.fill_exact_case(shape, dtype, kind)


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_fill_structure(dtype):
    PC.fill_structure_case((131, 257), dtype)


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', PC.REAL_SHAPES, ids=PC.shape_id)
def test_fill_real_valued_data_under_the_derived_bound(shape, dtype):
    PC.fill_real_case(shape, dtype, 'emulator')


def test_fill_refusals_leave_everything_untouched():
    PC.fill_refusals_case()


@pytest.mark.parametrize('pair', PC.CAST_PAIRS, ids=['f64_f32', 'f32_f64', 'f32_f32', 'f64_f64'])
@pytest.mark.parametrize('shape', PC.SEAMS, ids=PC.shape_id)
def test_cast_is_numpys(shape, pair):
    PC.cast_case(shape, *pair)


def test_cast_specials_are_what_they_say():
    PC.cast_specials_are_covered()


def test_cast_refusals():
    PC.cast_refusals_case()


def test_host_rounding_helper_against_the_independent_statement():
    PC.host_helper_case()


@pytest.mark.parametrize('src', [F32, F64], ids=['f32', 'f64'])
def test_to_bf16_rounding_table(src):
    PC.to_bf16_table_case(src)


def test_to_bf16_copies_every_bf16_pattern():
    PC.to_bf16_copy_case()


@pytest.mark.parametrize('src', [F64, F32, BF16], ids=['f64', 'f32', 'bf16'])
@pytest.mark.parametrize('shape', PC.SEAMS, ids=PC.shape_id)
def test_to_bf16_layouts(shape, src):
    PC.to_bf16_layout_case(shape, src)


def test_to_bf16_refusals():
    PC.to_bf16_refusals_case()


def test_fill_uniform_with_padding_and_scale():
    PC.fill_uniform_case()


def test_report():
    """(runs last: the lines profiles/preprocess_ops.txt records -- wall time of the cases at the two large shapes, and the
    measured deviations of the real-valued fills next to their bounds)"""
    for t, name in sorted(TIMES, reverse=True)[:12]:
        print('emulator %6.2f s  %s' % (t, name))
    print('\n'.join(PC.REPORT))
