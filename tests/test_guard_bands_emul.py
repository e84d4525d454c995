"""The project's cases between guard bands on the host emulator (tests/guarded.py, tests/guard_band_cases.py): every
allocation of the package and of the case sits between two bands of 4096 bytes of 0xFF, and after the case -- which keeps its
own assertions -- every band must still hold them.  Plus the wrapper's own test: a byte written into a band is named."""
import numpy as np
import pytest

from emul.runtime import emulated_runtime, use_runtime

import guard_band_cases as GB
from guarded import GuardedMemory, guarded


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


def three_buffers(rt):
    mem = GuardedMemory(rt.mem, band=4096)
    bufs = [mem.empty(100), mem.from_host(np.arange(77, dtype=np.float64)), mem.empty(1000)]
    assert all(b.ptr % 256 == 0 for b in bufs) and [b.nbytes for b in bufs] == [100, 616, 1000]
    np.testing.assert_array_equal(mem.to_host(bufs[1], (77,), np.float64), np.arange(77.0))
    return mem, bufs


def wrapper_names_the_damaged_band(rt, poke):
    """Three buffers; untouched they pass.  Then one byte of one band is overwritten through the inner allocation's own
    array / tensor (`poke(owner, index, value)`: a write inside that allocation) and check() must name exactly that buffer,
    side and offset -- for the band after a buffer and for the band before one."""
    mem, bufs = three_buffers(rt)
    assert mem.check() == 6 and mem.records == []
    for side, offset in (('after', 616 + 5), ('before', -3)):
        mem, bufs = three_buffers(rt)
        poke(mem.records[1].inner.owner, 4096 + offset, 0x5A)
        with pytest.raises(AssertionError) as err:
            mem.check()
        msg = str(err.value)
        assert msg.count('buffer #') == 1 and 'buffer #2 (616 bytes, tests/test_guard_bands_emul.py:' in msg, msg
        assert 'three_buffers <- ' in msg, msg              # the allocation site: here the test itself allocates
        assert 'band %s damaged at offsets %d..%d (1 bytes), first bytes 5a' % (side, offset, offset) in msg, msg


def test_wrapper_names_the_damaged_band(emul):
    def poke(owner, index, value):
        owner[index] = value
    wrapper_names_the_damaged_band(emul, poke)


def test_guarded_reports_damage_and_the_failure_of_the_body(emul):
    with pytest.raises(AssertionError, match='band after damaged at offsets 8..8') as err:
        with guarded(emul) as g:
            buf = g.mem.empty(8)
            g.mem.records[0].inner.owner[4096 + 8] = 0
            raise ValueError('the body failed too')
    assert 'the body failed too' in str(err.value)
    with guarded(emul) as g:
        g.mem.empty(8)
    assert (g.buffers, g.bands) == (1, 2)
    del buf


def test_allocation_site_is_the_package_frame(emul):
    """An allocation made by the package is recorded with the package's own two innermost frames, not the test's."""
    from skfusion_amd._engine import upload_matrix
    with guarded(emul) as g:
        upload_matrix(np.ones((3, 4)), 'f64')
        site = g.mem.records[-1].site
    assert site.startswith('scikit-fusion_amd/_engine.py:') and ' upload_matrix' in site and 'test_' not in site, site


@pytest.mark.parametrize('case', [c[0] for c in GB.CASES])
def test_case_leaves_every_band_intact(case, monkeypatch):
    GB.run_guarded(case, monkeypatch, 'emulator')
