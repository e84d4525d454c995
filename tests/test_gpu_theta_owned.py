"""Sparse constraints of ownership-sharded fits as the CSR of every rank's owned rows (SKF_OPT_THETA_OWNED_ROWS,
`shard='owned'`) on the MI355X: the cases of tests/theta_owned_cases.py -- hub rows below, across and beyond one 64-column
group, split and unsplit, worlds of 2 and 3, every engine.  The ranks of a group are threads of this process on the one
device (helpers.ThreadGroup)."""
import pytest

import skfusion_amd._native as nat

import theta_owned_cases as TO

pytestmark = pytest.mark.gpu


def test_creation_of_owned_constraint_slices():
    rt = nat.get_runtime()
    TO.creation_cases(rt.lib, rt.mem.empty(4096).ptr)


@pytest.mark.parametrize('size', [2, 3])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_bound_lists_of_every_rank_equal_scipy_rows_of_its_slice(dtype, size, monkeypatch):
    assert not TO.lists_case(dtype, size, monkeypatch)


def test_bound_lists_with_a_rank_that_owns_no_row(monkeypatch):
    assert TO.lists_case('bf16', 3, monkeypatch, n=120)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_lists_of_a_dense_fed_compacted_constraint(dtype, monkeypatch):
    TO.dense_fed_lists_case(dtype, monkeypatch)


@pytest.mark.parametrize('which', ['offset', 'range', 'descending'])
def test_invalid_slices_are_refused_by_the_device_check(which):
    TO.invalid_slice_case(which)


@pytest.mark.parametrize('hub', [64, 0])
@pytest.mark.parametrize('size', [2, 3])
@pytest.mark.parametrize('c', [5, 65, 130])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_constraint_slices_give_the_bits_of_the_dense_fed_owned_fit(dtype, c, size, hub, monkeypatch):
    TO.hub_bits_case(dtype, c, size, hub, monkeypatch)


@pytest.mark.parametrize('size', [2, 3])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_split_rows_on_both_sides_of_every_boundary(dtype, size, monkeypatch):
    TO.hub_bits_case(dtype, 65, size, 64, monkeypatch, lengths=TO.SPREAD_LENGTHS)


def test_dfmc_constraint_slices_give_the_bits_of_the_dense_fed_owned_fit(monkeypatch):
    TO.dfmc_bits_case(2, monkeypatch)


@pytest.mark.parametrize('size', [2, 3])
@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_both_forms_launch_the_same_kernels(dtype, size, monkeypatch):
    TO.launch_counts_case(dtype, size, monkeypatch)


@pytest.mark.parametrize('size', [2, 3])
def test_owned_fit_with_constraint_slices_against_the_oracle(size, monkeypatch):
    TO.oracle_case(size, monkeypatch)


def test_a_slice_denser_than_the_density_rule_against_the_oracle(monkeypatch):
    TO.oracle_case(2, monkeypatch, lengths=TO.DENSE_LENGTHS)


def test_owned_plans_never_expand_their_constraint(monkeypatch):
    TO.never_expanded_plans(monkeypatch)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('cls_name', ['Dfmf', 'Dfmc'])
def test_api_owned_fits_never_expand_the_constraint(cls_name, dtype, monkeypatch):
    TO.api_case(cls_name, dtype, monkeypatch)


def test_functional_seams_take_entries_for_owned_fits_only():
    TO.functional_seam_case()
