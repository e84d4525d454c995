"""Plans on the edges of the split-K decision on the MI355X: tests/slicing_cases.py (the emulator's cases and the relation
time model, which needs relations of ~4000 rows)."""
import pytest

import slicing_cases as SC

pytestmark = pytest.mark.gpu

CASES = sorted(SC.EDGES.items()) + sorted(SC.GPU_ONLY.items())


@pytest.mark.parametrize('name,case', CASES, ids=[c[0] for c in CASES])
def test_plans_on_the_edges_of_the_slicing_decision(name, case, monkeypatch):
    SC.slicing_case(case, 'GPU slicing ' + name, monkeypatch)
