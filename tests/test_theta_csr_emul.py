"""Sparse constraints given as their entries (skf_theta_desc.data == NULL, skf_plan_set_constraint_entries) and the hub-row
split of the sparse constraint pass on the host emulator: entries-fed against dense-fed bit for bit on every schedule, the
list path without a dense twin, hub rows cut into segments, every refusal, and the public API (tests/theta_csr_cases.py)."""
import ctypes as C
import os

import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import theta_csr_cases as TC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


@pytest.mark.parametrize('c', [8, 20])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_entries_equal_dense_small_graph_schedule(dtype, c, monkeypatch):
    TC.entries_against_dense('dfmf', dtype, c, monkeypatch, expect_small=True)


@pytest.mark.parametrize('dtype,c,general', [('f64', 70, False), ('f32', 20, True), ('bf16', 8, False), ('bf16', 70, False)])
def test_entries_equal_dense_general_schedule(dtype, c, general, monkeypatch):
    TC.entries_against_dense('dfmf', dtype, c, monkeypatch, general=general, expect_small=False)


def test_entries_equal_dense_valu_engine(monkeypatch):
    TC.entries_against_dense('dfmf', 'f32', 20, monkeypatch, general=True, engine=nat.SKF_ENGINE_VALU)


@pytest.mark.parametrize('dtype,c', [('f64', 20), ('bf16', 70)])
def test_entries_equal_dense_dfmc(dtype, c, monkeypatch):
    TC.entries_against_dense('dfmc', dtype, c, monkeypatch)


@pytest.mark.parametrize('dtype,c', [('f64', 8), ('f32', 70)])
def test_entries_equal_dense_fold_in(dtype, c, monkeypatch):
    TC.entries_against_dense('transform', dtype, c, monkeypatch)


def test_batched_restarts_share_the_entries():
    TC.batch_case('f64')


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_half_full_constraint_stays_lists(dtype):
    TC.half_full_case(dtype, 'emulator')


@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_all_zero_constraint(dtype, monkeypatch):
    TC.all_zero_case(dtype, monkeypatch)


@pytest.mark.parametrize('c', [5, 65])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_hub_rows_split(dtype, c, monkeypatch):
    TC.hub_case(dtype, c, monkeypatch, n=150)


def test_hub_rows_on_both_sides_of_an_owner_boundary(monkeypatch):
    TC.hub_owned_case(monkeypatch, c=5, n=300)


@pytest.mark.parametrize('which', TC.BROKEN + ('handover', 'ok'))
def test_broken_lists_are_refused_at_bind_before_any_gather(which):
    TC.refusal_case(which)


def test_setter_state_and_range():
    TC.setter_state_case()


def test_creation_checks_need_no_device():
    """The product library (cross-compiled for gfx950), no device: the plan-creation checks answer before any HIP call."""
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load_library()
    keep = (C.c_uint8 * 4096)()
    TC.creation_cases(lib, C.addressof(keep))


def test_api_constraint_entries(monkeypatch):
    TC.api_constraint_entries_case(monkeypatch)


@pytest.mark.parametrize('cls,dtype', [('Dfmf', 'f64'), ('Dfmf', 'f32'), ('Dfmc', 'f64')])
def test_api_fit_never_expands(cls, dtype, monkeypatch):
    TC.api_fit_case(cls, dtype, monkeypatch)


@pytest.mark.parametrize('n_run', [1, 2])
def test_api_fold_in_never_expands(n_run, monkeypatch):
    TC.api_transform_case('f64', monkeypatch, n_run=n_run)


def test_api_rule_and_switches(monkeypatch):
    TC.api_rule_case(monkeypatch)


def test_api_restarts_share_launches(monkeypatch):
    TC.api_restarts_case('f64', monkeypatch)


def test_api_save_and_load(tmp_path, monkeypatch):
    TC.api_save_load_case(tmp_path, monkeypatch)
