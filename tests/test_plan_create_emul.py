"""Every refusal of skf_plan_create by status and full text, and which one answers where two apply, on the host emulator
(tests/plan_create_cases.py).  No kernel is launched."""
import pytest

from emul.runtime import emulated_runtime, use_runtime

import plan_create_cases as PC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import launch_count
    with use_runtime(emulated_runtime()) as rt:
        before = launch_count()
        yield rt
        assert launch_count() == before


@pytest.mark.parametrize('name', list(PC.REFUSALS))
def test_refusal_by_status_and_text(name, emul):
    PC.refusal_case(emul.lib, name)


def test_null_arrays_are_refused(emul):
    PC.null_array_cases(emul.lib)


@pytest.mark.parametrize('name', list(PC.ACCEPTED))
def test_the_descriptors_the_cases_start_from_are_accepted(name, emul):
    PC.accepted_case(emul.lib, name)
