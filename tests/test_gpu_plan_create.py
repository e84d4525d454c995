"""Every refusal of skf_plan_create by status and full text, and which one answers where two apply, against the product
library -- the table of tests/plan_create_cases.py as another compiler built it.  Create, query and destroy only: no kernel
is launched."""
import pytest

import skfusion_amd._native as nat

import plan_create_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from skfusion_amd._engine import launch_count
    rt = nat.get_runtime()
    before = launch_count(rt)
    yield rt.lib
    assert launch_count(rt) == before


@pytest.mark.parametrize('name', list(PC.REFUSALS))
def test_refusal_by_status_and_text(name, lib):
    PC.refusal_case(lib, name)


def test_null_arrays_are_refused(lib):
    PC.null_array_cases(lib)


@pytest.mark.parametrize('name', list(PC.ACCEPTED))
def test_the_descriptors_the_cases_start_from_are_accepted(name, lib):
    PC.accepted_case(lib, name)
