"""One dense iteration of every engine on the hardware, stage by stage against the host model of tests/dense_cases.py
(the error model behind every bound is its module comment): the contractions, the backbone in the device's own W form, the
per-element update from the device's P, Q, S, the DFMC completion (per-tile lists and mask blend, masked store) and, in
the second iteration, the contractions over the refreshed G^T.  Schedules: relation pipeline, staged, the three
small-graph launches and SKF_NO_SMALL_FUSED; object counts 1 .. 4099 off multiples of 4 / 8 / 64 / 128 / 256, ranks 1, 5,
8, 16, 64, 65, 128, 256, 320."""
import pytest

import dense_cases as DC

pytestmark = pytest.mark.gpu

CASES = DC.gpu_cases()


@pytest.mark.parametrize('name,case', CASES, ids=[c[0] for c in CASES])
def test_dense_iteration_against_host_model(name, case, monkeypatch):
    dtype, schedule, n, ranks, rels, thetas, kw = case
    DC.dense_case(dtype, schedule, n, ranks, rels, thetas, 'GPU ' + name, monkeypatch, **kw)
