"""The operators that touch a relation before the engine does -- skf_fill_unknown, skf_cast, skf_to_bf16, skf_fill_uniform
(tests/preprocess_cases.py) -- on the MI355X, through the C ABI, between guard bands: every shape of SEAMS, the structure
cases at 8209 x 67 and 131 x 257, the real-valued fills under their derived bound, the rounding table of every bf16 pattern
in both layouts, every refusal, and the transposed conversion of 2 097 185 rows, whose grid is 65 537 tiles high."""
import pytest

import skfusion_amd._native as nat

import preprocess_cases as PC

pytestmark = pytest.mark.gpu
F64, F32, BF16 = nat.SKF_F64, nat.SKF_F32, nat.SKF_BF16


def test_the_model_is_the_reference():
    assert PC.model_against_golden() > 800


@pytest.mark.parametrize('kind', PC.KINDS)
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', PC.SEAMS, ids=PC.shape_id)
def test_fill_exact_data_byte_for_byte(shape, dtype, kind):
    PC.fill_exact_case(shape, dtype, kind)


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', PC.STRUCTURE_SHAPES, ids=PC.shape_id)
def test_fill_structure(shape, dtype):
    PC.fill_structure_case(shape, dtype)


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', PC.REAL_SHAPES, ids=PC.shape_id)
def test_fill_real_valued_data_under_the_derived_bound(shape, dtype):
    PC.fill_real_case(shape, dtype, 'gpu')


def test_fill_refusals_leave_everything_untouched():
    PC.fill_refusals_case()


@pytest.mark.parametrize('pair', PC.CAST_PAIRS, ids=['f64_f32', 'f32_f64', 'f32_f32', 'f64_f64'])
@pytest.mark.parametrize('shape', PC.SEAMS, ids=PC.shape_id)
def test_cast_is_numpys(shape, pair):
    PC.cast_case(shape, *pair)


def test_cast_refusals():
    PC.cast_refusals_case()


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


def test_to_bf16_transposed_past_65535_row_tiles():
    PC.y_extent_case()


def test_fill_uniform_with_padding_and_scale():
    PC.fill_uniform_case()


def test_report():
    """(runs last: the measured deviations of the real-valued fills next to their bounds, as profiles/preprocess_ops.txt
    records them)"""
    print('\n'.join(PC.REPORT))
