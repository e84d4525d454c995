"""The column-mean initialisers on the device (csrc/skf_init.h, skf_plan_relation_norms, skf_plan_init_column_means,
`init_device` of Dfmf / Dfmc) on the host emulator: the small subset of tests/init_device_cases.py -- exact data byte for
byte against `_init.initialize` in every engine and stored form, the pools of `random_c`, the line norms, real-valued data
under the derived bound (and the bound itself on the CPU), every refusal under guard bands, the public API."""
import ctypes as C
import os

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import init_device_cases as IC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
@pytest.mark.parametrize('form', ['dense', 'csr'])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_exact_byte_for_byte(dtype, form, init_type):
    IC.exact_case(dtype, (67, 131, 40), (5, 7, 5), 'ratings', form, init_type)


@pytest.mark.parametrize('kind', ['binary', 'ones'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_exact_zero_one_relations(dtype, kind):
    """SKF_BF16 keeps these as bitmaps (the sparse one as lists of its ones beside it); columns tie heavily."""
    IC.exact_case(dtype, (67, 131, 40), (5, 7, 5), kind, 'dense', 'random_c')


def test_exact_wider_ranks_and_several_tiles():
    IC.exact_case('f32', (203, 997, 67), (64, 65, 64), 'ratings', 'dense', 'random_vcol')
    IC.exact_case('bf16', (203, 997, 67), (64, 65, 64), 'binary', 'dense', 'random_c')


@pytest.mark.parametrize('dtype,kind,form', [('f64', 'ratings', 'dense'), ('f32', 'ratings', 'csr'), ('bf16', 'ratings', 'dense'),
                                             ('bf16', 'binary', 'dense')])
def test_norms_exact_over_several_slabs(dtype, kind, form):
    IC.norms_case(dtype, (600, 131, 300), kind, form)


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
def test_bound_holds_on_the_cpu(init_type):
    IC.bound_on_cpu_case((203, 997, 67), (5, 7, 5), init_type)


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
@pytest.mark.parametrize('dtype,form', [('f64', 'dense'), ('f32', 'dense'), ('f64', 'csr')])
def test_real_data_under_the_derived_bound(dtype, form, init_type):
    IC.real_case(dtype, (67, 131, 40), (5, 7, 5), form, init_type)


def test_refusals_and_guards():
    IC.refusals_case('f32')
    IC.refusals_case('bf16')


def test_refusals_need_no_device():
    """The product library (cross-compiled for gfx950), no device: these checks answer before any HIP call."""
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load_library()
    keep = (C.c_uint8 * 4096)()
    IC.refusals_without_device(lib, (C.addressof(keep) + 255) // 256 * 256)


@pytest.mark.parametrize('cls,dtype,kind,init_type', [('Dfmf', 'f64', 'dense', 'random_c'), ('Dfmf', 'f32', 'sparse', 'random_vcol'),
                                                      ('Dfmf', 'bf16', 'binary', 'random_c'), ('Dfmc', 'f32', 'dense', 'random_c'),
                                                      ('Dfmc', 'f64', 'sparse', 'random_c')])
def test_public_api_equals_the_host_initialiser(cls, dtype, kind, init_type, monkeypatch):
    IC.api_case(cls, dtype, kind, init_type, monkeypatch)


@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_public_api_restarts(dtype, monkeypatch):
    """n_run = 3 with n_jobs = 2: shared launches of a small graph (f64) / one plan per restart (bf16)."""
    IC.api_case('Dfmf', dtype, 'dense', 'random_c', monkeypatch, n_run=3, n_jobs=2)


@pytest.mark.parametrize('cls,what', [('Dfmc', 'masked'), ('Dfmf', 'narrow'), ('Dfmf', 'random')])
def test_ineligible_fits_stay_on_the_host(cls, what):
    IC.ineligible_case(cls, what)


def test_device_fill_with_the_default_initialiser(monkeypatch):
    IC.device_fill_case('f64', monkeypatch)
