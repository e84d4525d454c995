"""The column-mean initialisers on the device for relations with missing values (skf_plan_relation_norms_filled,
skf_plan_init_column_means_filled, `init_device` of Dfmf / Dfmc on ``unstored='unknown'`` relations) on the host emulator: the
small subset of tests/init_known_cases.py -- exact data byte for byte against `_init.initialize` in every engine, both
initialisers and both list forms, hand-made selections and the mixed type in both view orders, the line norms, mask-fed
against CSR-fed, real-valued data under the derived bound (the host initialiser held to it too), every refusal under guard
bands, the public API."""
import ctypes as C
import os

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import init_known_cases as KC

SMALL = (67, 131, 40)


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
@pytest.mark.parametrize('form,fill', [('known', 2.5), ('rank1', 2.5), ('rank1', 'mean'), ('rank1', 'row_mean'), ('rank1', 'col_mean')])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_exact_byte_for_byte(dtype, form, fill, init_type):
    KC.exact_case(dtype, SMALL, (5, 7, 5), form, fill, init_type)


@pytest.mark.parametrize('form,fill', [('known', 2.5), ('rank1', 'mean')])
def test_exact_empty_and_full_columns(form, fill):
    """The pattern transposed: the empty and the full line are columns of the relation."""
    KC.exact_case('f32', SMALL, (5, 7, 5), form, fill, 'random_c', flip=True)


def test_exact_ranks_across_the_lane_blocks():
    """Ranks 64 and 65 (one and two factor columns per lane), 128 and 200 (two and four)."""
    KC.exact_case('f32', (203, 997, 67), (64, 65, 64), 'known', 2.5, 'random_vcol')
    KC.exact_case('f64', (203, 997, 67), (128, 200, 128), 'rank1', 'row_mean', 'random_vcol')


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_no_stored_entry_at_all(dtype):
    KC.exact_case(dtype, SMALL, (5, 7, 5), 'known', 2.5, 'random_c', empty=True)


@pytest.mark.parametrize('form,fill', [('known', 2.5), ('rank1', 2.5), ('rank1', 'col_mean')])
@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_chosen_by_all_chosen_by_none_and_both_view_orders(dtype, form, fill):
    KC.chosen_columns_case(dtype, form, fill)


@pytest.mark.parametrize('form,fill,flip', [('known', 2.5, False), ('known', 2.5, True), ('rank1', 'mean', False), ('rank1', 'mean', True),
                                            ('rank1', 'row_mean', False), ('rank1', 'col_mean', False)])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_line_norms_exact(dtype, form, fill, flip):
    KC.norms_case(dtype, (600, 131, 300), form, fill, flip)


@pytest.mark.parametrize('form', ['dense', 'csr'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_older_forms_take_the_unchanged_route(dtype, form):
    KC.unchanged_route_case(dtype, form)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_mask_fed_equals_csr_fed(dtype):
    KC.mask_fed_case(dtype)


@pytest.mark.parametrize('form,fill', [('known', 'mean'), ('rank1', 'mean'), ('rank1', 'row_mean')])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_real_data_under_the_derived_bound(dtype, form, fill):
    KC.real_case(dtype, SMALL, (5, 7, 5), form, fill)


def test_refusals_and_guards():
    KC.refusals_case('f32')
    KC.refusals_case('bf16')


def test_refusals_need_no_device():
    """The product library (cross-compiled for gfx950), no device: these checks answer before any HIP call."""
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load_library()
    keep = (C.c_uint8 * 4096)()
    KC.refusals_without_device(lib, (C.addressof(keep) + 255) // 256 * 256)


@pytest.mark.parametrize('cls,dtype,fill,init_type', [('Dfmc', 'f64', 2.5, 'random_c'), ('Dfmf', 'f32', 2.5, 'random_c'),
                                                      ('Dfmf', 'f64', 'row_mean', 'random_vcol'), ('Dfmc', 'bf16', 2.5, 'random_vcol'),
                                                      ('Dfmc', 'f32', 'row_mean', 'random_c')])
def test_public_api_equals_the_host_initialiser(cls, dtype, fill, init_type, monkeypatch):
    KC.api_case(cls, dtype, fill, init_type, monkeypatch)


def test_public_api_restarts(monkeypatch):
    KC.api_case('Dfmc', 'f64', 2.5, 'random_c', monkeypatch, n_run=3, n_jobs=2)
