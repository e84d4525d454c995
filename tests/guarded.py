"""Guard bands around every allocation of a runtime (TEST INFRASTRUCTURE, not a product path).

Every allocation of the package and of the tests goes through ``rt.mem.empty`` / ``rt.mem.from_host``.  ``GuardedMemory``
wraps a memory object (the emulator's HostMemory or the product's TorchDeviceMemory), asks it for ``band + n + band`` bytes,
fills both bands with 0xFF (NaN as bf16, f32 and f64) and hands the middle out.  ``check()`` reads every band back: a byte
that is no longer 0xFF is a store outside a buffer.  A read past a buffer that reaches a result turns it into NaN and fails
the case's own comparison.  ``with guarded(): <case>`` runs a case of the suite on such a runtime.

What it proves: no write within `band` bytes outside any buffer on the paths run under it.  What it does not: stores
farther away than that."""
import contextlib
import os
import sys

import numpy as np

import skfusion_amd._native as nat

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 0xFF
CHECKED = []                    # (label, buffers, bands) of every guarded() block of this session, in order


PACKAGE = os.path.dirname(os.path.abspath(nat.__file__))


def _is_package_frame(filename):
    return os.path.abspath(filename).startswith(PACKAGE + os.sep)


def _site():
    """'file:line function' of the two innermost frames of the allocation that are not test code (the package's own); of
    the two innermost frames outside this module where the test allocates directly."""
    frames = []
    f = sys._getframe(1)
    while f is not None:
        if os.path.abspath(f.f_code.co_filename) != os.path.abspath(__file__):
            frames.append(f)
        f = f.f_back
    own = [f for f in frames if _is_package_frame(f.f_code.co_filename)]
    pick = (own or frames)[:2]
    return ' <- '.join('%s:%d %s' % (os.path.relpath(os.path.realpath(f.f_code.co_filename), os.path.realpath(os.path.dirname(HERE))), f.f_lineno,
                                     f.f_code.co_name) for f in pick)


class _Record(object):
    __slots__ = ('serial', 'n', 'site', 'inner')

    def __init__(self, serial, n, site, inner):
        self.serial, self.n, self.site, self.inner = serial, n, site, inner


class GuardedMemory(object):
    def __init__(self, inner, band=4096):
        assert band > 0 and band % 256 == 0
        self.inner, self.band = inner, band
        self.records = []
        self._serial = 0

    def __getattr__(self, name):            # stream, new_stream, stream_scope, torch, device, ...
        return getattr(self.inner, name)

    def _wrap(self, raw, n):
        band = self.band
        assert raw.ptr % 256 == 0
        self._serial += 1
        self.records.append(_Record(self._serial, n, _site(), raw))
        return nat.Buffer(raw.ptr + band, n, raw.owner[band:band + n])

    def empty(self, nbytes):
        n, band = int(nbytes), self.band
        raw = self.inner.empty(band + n + band)
        owner = raw.owner
        if isinstance(owner, np.ndarray):
            owner[:band] = FILL
            owner[band + n:band + n + band] = FILL
        else:                               # a torch tensor: the fill runs on torch's stream, the engine on its own
            owner[:band].fill_(FILL)
            owner[band + n:band + n + band].fill_(FILL)
            self.inner.synchronize()
        return self._wrap(raw, n)

    def from_host(self, array, sync=True):
        a = np.ascontiguousarray(array)
        n, band = a.nbytes, self.band
        padded = np.full(band + n + band, FILL, dtype=np.uint8)
        padded[band:band + n] = a.view(np.uint8).reshape(-1)
        return self._wrap(self.inner.from_host(padded, sync), n)

    def to_host(self, buf, shape, dtype):
        return self.inner.to_host(buf, shape, dtype)

    def synchronize(self):
        return self.inner.synchronize()

    def as_tensor(self, buf, offset, nbytes, np_dtype):
        return self.inner.as_tensor(buf, offset, nbytes, np_dtype)

    def _bands(self):
        """(records, uint8 array of shape (len(records), 2, band)) read back after a synchronize."""
        self.inner.synchronize()
        band, recs = self.band, self.records
        if not recs:
            return recs, np.zeros((0, 2, band), np.uint8)
        if isinstance(recs[0].inner.owner, np.ndarray):
            got = np.stack([np.stack([r.inner.owner[:band], r.inner.owner[band + r.n:band + r.n + band]]) for r in recs])
        else:
            import torch
            parts = []
            for r in recs:
                parts += [r.inner.owner[:band], r.inner.owner[band + r.n:band + r.n + band]]
            got = torch.cat(parts).cpu().numpy().reshape(len(recs), 2, band)
        return recs, got

    def check(self):
        """Raise AssertionError naming every damaged band; return the number of bands checked.  The checked buffers are
        released."""
        recs, got = self._bands()
        bad = []
        for r, pair in zip(recs, got):
            for side, bytes_ in zip(('before', 'after'), pair):
                hit = np.flatnonzero(bytes_ != FILL)
                if hit.size:
                    # offsets are relative to the buffer: negative in the band before it, from n on in the band after
                    base = -self.band if side == 'before' else r.n
                    bad.append('buffer #%d (%d bytes, %s): band %s damaged at offsets %d..%d (%d bytes), first bytes %s'
                               % (r.serial, r.n, r.site, side, base + hit[0], base + hit[-1], hit.size,
                                  ' '.join('%02x' % b for b in bytes_[hit[:16]])))
        n = 2 * len(recs)
        self.records = []
        assert not bad, 'stores outside a buffer:\n  ' + '\n  '.join(bad)
        return n


class Checked(object):
    """What a guarded() block yields: .rt the guarded runtime, .mem its memory, .bands / .buffers filled at exit."""
    def __init__(self, rt):
        self.rt, self.mem, self.bands, self.buffers = rt, rt.mem, 0, 0


@contextlib.contextmanager
def guarded(rt=None, band=4096, label=None):
    """Run the body on `rt` (default: the current runtime) with guard bands around every allocation; check them at the
    end, also when the body raised (both failures are reported)."""
    from emul.runtime import use_runtime
    if rt is None:
        rt = nat.get_runtime()
    mem = GuardedMemory(rt.mem, band)
    res = Checked(nat.Runtime(rt.lib, mem, rt.name))
    with use_runtime(res.rt):
        try:
            yield res
        except BaseException as exc:
            try:
                mem.check()
            except AssertionError as damage:
                raise AssertionError('%s\n(the guarded body also failed: %r)' % (damage, exc)) from exc
            raise
        res.buffers = len(mem.records)
        res.bands = mem.check()
    if label is None:
        label = os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]
    CHECKED.append((label, res.buffers, res.bands))
    print('guarded %s %s: %d buffers, %d bands intact' % (rt.name, label, res.buffers, res.bands))
