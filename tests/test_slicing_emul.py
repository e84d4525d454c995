"""Plans on the edges of the split-K decision on the CPU (host SIMT emulator): tests/slicing_cases.py."""
import pytest

from emul.runtime import emulated_runtime, use_runtime
import slicing_cases as SC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0        # no split-K launch of the module outgrew the scratch its plan sized


@pytest.mark.parametrize('name', sorted(SC.EDGES))
def test_plans_on_the_edges_of_the_slicing_decision(name, emul, monkeypatch):
    SC.slicing_case(SC.EDGES[name], 'emulator slicing ' + name, monkeypatch, emul)
