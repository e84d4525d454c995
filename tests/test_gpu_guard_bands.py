"""The project's cases between guard bands on the MI355X (tests/guarded.py, tests/guard_band_cases.py): every allocation of
the package and of the case is the middle of a torch allocation whose first and last 4096 bytes hold 0xFF, and after the case
-- which keeps its own assertions -- every band must still hold them.  The bands lie inside the allocations, so no access of
these tests leaves memory that torch handed out.  Plus the wrapper's own test on device memory."""
import pytest

import skfusion_amd._native as nat

import guard_band_cases as GB
from test_guard_bands_emul import wrapper_names_the_damaged_band

pytestmark = pytest.mark.gpu


def test_wrapper_names_the_damaged_band():
    rt = nat.get_runtime()

    def poke(owner, index, value):
        owner[index] = value                       # a one-byte tensor assignment inside the inner allocation
        rt.mem.synchronize()
    wrapper_names_the_damaged_band(rt, poke)


@pytest.mark.parametrize('case', [c[0] for c in GB.CASES if c[1] == 'both'])
def test_case_leaves_every_band_intact(case, monkeypatch):
    GB.run_guarded(case, monkeypatch, 'GPU')
