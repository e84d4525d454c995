"""The consuming side of a fitted model on the device: blockwise reconstruction (``DeviceReconstructor``), the product of the
backbones along a chain (``chain_backbone``) and the completion operators that never form the dense product
(``DeviceCompleter``, csrc/skf_complete.h).  Everything here works from factors that are already fitted; the plan of a fit is
``_engine``'s subject, and ``_engine`` imports these names from here (this module needs ``_native`` and numpy only).
"""
import contextlib
import ctypes as C

import numpy as np

from . import _native as nat


class DeviceMatrix(object):
    """A row-major matrix that already lives in HBM (engine dtype), e.g. synthetic benchmark
    data generated on the device with ``fill_uniform``.  (Defined on this side because ``DeviceReconstructor.block`` hands
    one out; the engine takes it from here.)"""

    def __init__(self, buf, shape, ld=None, binary=False):
        self.buf, self.shape, self.ld = buf, tuple(shape), ld if ld is not None else shape[1]
        self.binary = bool(binary)      # the caller's promise that every entry is 0 or 1 (SKF_REL_BINARY; checked at bind)
        self.nnz = 0                    # constraints: an upper bound on the non-zero entries (0 = unknown / dense)
        self.known = 0                  # byte masks in HBM: the number of KNOWN entries (mask == 0); 0 = not counted

    def rows(self, begin, count, itemsize):
        """View of `count` rows from `begin` on (no copy; the parent buffer stays referenced)."""
        return DeviceMatrix(_BufferView(self.buf, begin * self.ld * itemsize), (count, self.shape[1]), self.ld,
                            self.binary)


class _BufferView(object):
    def __init__(self, parent, offset):
        self.parent, self.ptr = parent, parent.ptr + offset


class _ResidentFactors(object):
    """``S`` and the column factor in the master type of ``dtype`` ('bf16' works on the f32 masters), uploaded ONCE and kept
    in HBM across the blocks: what ``DeviceReconstructor`` and ``DeviceCompleter`` are built on."""

    def __init__(self, S, G_col, dtype, runtime, what, G_col_device=None):
        self.rt = runtime or nat.get_runtime()
        code = nat.DTYPES[dtype]
        self.code = nat.SKF_F32 if code == nat.SKF_BF16 else code
        self.npd = nat.NP_DTYPE[self.code]
        self.es = np.dtype(self.npd).itemsize
        Sm = np.ascontiguousarray(S, dtype=self.npd)
        B = None if G_col is None else np.ascontiguousarray(G_col, dtype=self.npd)
        if Sm.ndim != 2 or (B is not None and (B.ndim != 2 or B.shape[1] != Sm.shape[1])):
            raise ValueError('shape mismatch in ' + what)
        self.ci, self.cj = Sm.shape
        self.nj = self.cj if B is None else B.shape[0]          # columns of a block
        self.s = self.rt.mem.from_host(Sm)
        shared = B is not None and G_col_device is not None
        self.b = None if B is None else (G_col_device if shared else self.rt.mem.from_host(B))
        self.uploads = 1 if (B is None or shared) else 2   # H2D copies of S / G_col so far (does not grow with the block count)


class DeviceReconstructor(_ResidentFactors):
    """R_hat blocks = G_row[block] @ S @ G_col.T on the device (two strided MFMA GEMMs through ``skf_gemm``) with
    ``S`` and the column factor uploaded ONCE and kept resident across blocks -- the building block of
    ``FusionFit.complete_blocks`` for relations whose dense reconstruction does not fit on the host in one
    piece (reference base.py:119-146 materialises the whole product) and of the chained latent profiles
    (f4: ``S`` is then the product of the backbones along a ``chain()`` path).  ``G_col=None``: blocks are
    ``G_row[block] @ S`` (the profile form of reference examples/pharma_chaining.py:43-53, one GEMM)."""

    def __init__(self, S, G_col=None, dtype='f64', runtime=None, G_col_device=None):
        """``G_col_device``: the buffer another reconstructor of the same dtype already uploaded for this column factor
        (``other.b`` with ``other.nj`` rows: several paths that end in one object type share one copy in HBM)."""
        _ResidentFactors.__init__(self, S, G_col, dtype, runtime, 'reconstruction', G_col_device)
        self._h = self._out = None
        self._rows = 0

    def _gemm(self, Ap, sa_m, sa_k, Bp, sb_k, sb_n, Cp, ldc, M, N, K):
        _device_gemm(self.rt, self.code, Ap, sa_m, sa_k, Bp, sb_k, sb_n, Cp, ldc, M, N, K)

    def block(self, G_row_block, device=False):
        """Reconstruction of the rows of this block: a host ndarray (float64), or -- device=True -- a
        DeviceMatrix of the engine dtype that is valid until the next call (no D2H copy at all)."""
        A = np.ascontiguousarray(G_row_block, dtype=self.npd)
        if A.ndim != 2 or A.shape[1] != self.ci:
            raise ValueError('shape mismatch in reconstruction')
        m = A.shape[0]
        mem = self.rt.mem
        if m > self._rows:                     # scratch grows to the largest block seen, then is reused
            self._h = mem.empty(m * self.cj * self.es)
            self._out = self._h if self.b is None else mem.empty(m * self.nj * self.es)
            self._rows = m
        a = mem.from_host(A)
        self._gemm(a.ptr, self.ci, 1, self.s.ptr, self.cj, 1, self._h.ptr, self.cj, m, self.cj, self.ci)      # H = G_blk S
        if self.b is not None:
            self._gemm(self._h.ptr, self.cj, 1, self.b.ptr, 1, self.cj, self._out.ptr, self.nj, m, self.nj, self.cj)   # H G_col^T
        mem.synchronize()
        if device:
            return DeviceMatrix(self._out, (m, self.nj))
        return mem.to_host(self._out, (m, self.nj), self.npd).astype(np.float64)


def _device_gemm(rt, code, Ap, sa_m, sa_k, Bp, sb_k, sb_n, Cp, ldc, M, N, K):
    """C[M x N] = A[M x K] B[K x N] through skf_gemm (strides in elements; matrix-core GEMM of the master type `code`)."""
    d = nat.GemmDesc()
    d.A, d.B, d.C = Ap, Bp, Cp
    d.sa_m, d.sa_k, d.sb_k, d.sb_n, d.ldc, d.ldc2 = sa_m, sa_k, sb_k, sb_n, ldc, ldc
    d.M, d.N, d.K = M, N, K
    d.splits, d.a_dtype, d.b_dtype = 1, -1, -1
    rt.call('skf_gemm', code, nat.SKF_ENGINE_MFMA, C.byref(d), None, 0, rt.mem.stream)


def chain_backbone(backbones, runtime=None):
    """Product of the backbones along one `chain()` path, S_01 S_12 ... (c_first x c_last), on the device in f64 whatever
    the engine dtype (c x c work; the profile built from it inherits every digit lost here) -- left to right, the order of
    `reduce(np.dot, cf)` in reference examples/dicty_chaining.py:43-45 / pharma_chaining.py:46-47.  Returns a float64
    ndarray; an empty path has no backbone (the caller uses the factor itself)."""
    rt = runtime or nat.get_runtime()
    mats = [np.ascontiguousarray(S, dtype=np.float64) for S in backbones]
    if not mats:
        raise ValueError('an empty path has no backbone')
    for a, b in zip(mats[:-1], mats[1:]):
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[0]:
            raise ValueError('backbones along the path do not chain: %r then %r' % (a.shape, b.shape))
    if len(mats) == 1:
        return mats[0].copy()
    mem = rt.mem
    ups = [mem.from_host(S, sync=False) for S in mats]          # every buffer lives until the last product is through:
    mem.synchronize()                                           # the launches run on the engine's stream, not torch's
    keep, acc, rows, inner = [], ups[0], mats[0].shape[0], mats[0].shape[1]
    for S, nxt in zip(mats[1:], ups[1:]):
        out = mem.empty(rows * S.shape[1] * 8)
        keep.append(out)
        _device_gemm(rt, nat.SKF_F64, acc.ptr, inner, 1, nxt.ptr, S.shape[1], 1, out.ptr, S.shape[1], rows, S.shape[1], inner)
        acc, inner = out, S.shape[1]
    mem.synchronize()
    return mem.to_host(acc, (rows, inner), np.float64)


def device_reconstruct(G_row_block, S, G_col, dtype='f64', runtime=None):
    """One block (S and G_col uploaded for this call only; `DeviceReconstructor` keeps them resident)."""
    return DeviceReconstructor(S, G_col, dtype, runtime).block(G_row_block)


class AboveLimit(ValueError):
    """``DeviceCompleter.above`` found more entries than the caller's ``max_entries`` allows; ``found`` is the count."""

    def __init__(self, found):
        ValueError.__init__(self, '%d entries at or above the threshold' % found)
        self.found = found


def digit_walk(counts, n):
    """One step of the radix select, a pure function of one pass's histogram: ``(digit, above)`` -- the bin that holds the
    ``n``-th candidate (1-based) when the bins are walked from the highest digit down, and the candidates in the bins above
    it.  With fewer than ``n`` candidates in the histogram: the lowest bin that holds one (the smallest candidates).  An empty
    histogram: ``(None, 0)``."""
    counts = np.asarray(counts, dtype=np.uint64).astype(object)      # Python integers: sums of uint64 counts cannot wrap
    above = 0
    last = None
    for d in range(len(counts) - 1, -1, -1):
        if counts[d] == 0:
            continue
        if above + counts[d] >= n:
            return d, int(above)
        above += counts[d]
        last = d
    if last is None:
        return None, 0
    return last, int(above - counts[last])


def score_of_key(key, np_dtype):
    """The score whose order-preserving key (csrc/skf_complete.h ``score_key``) is ``key``, as a scalar of ``np_dtype``."""
    bits = 8 * np.dtype(np_dtype).itemsize
    sign, ones = 1 << (bits - 1), (1 << bits) - 1
    u = key ^ sign if key & sign else key ^ ones
    return np.array([u], dtype=np.uint64).astype('u%d' % (bits // 8)).view(np_dtype)[0]


class DeviceCompleter(_ResidentFactors):
    """The consuming side of a completion model without the dense reconstruction: for ``X = G_row S G_col^T`` the ``k`` best
    columns of every row (``topk``), the predictions at given pairs (``entries``), the position of given pairs in
    their row's ranking (``ranks``), every pair at or above a threshold as CSR (``above``), the n-th largest score over all
    row blocks (``kth``, by counting passes ``digits``), every row's own k-th score for any k with the columns at or above
    it (``row_kth``, ``row_best``) and the histogram of every score by value with that of given pairs (``hist``,
    ``histogram``), all on the device (csrc/skf_complete.h).  The reference forms ``X`` on the host (fusion/base/base.py ``complete``) and its users rank or
    index that array (examples/movielens_completion.py:121-126).  ``S`` and ``G_col`` are uploaded ONCE and stay resident
    across blocks (the contract of ``DeviceReconstructor``); per block only ``H = G_row[block] S`` (``skf_gemm``), the
    block's exclusion lists, its outputs and the partial lists of the column splits live in HBM -- never anything of size
    ``n_i x n_j``.  ``dtype`` 'bf16' scores in f32 on the f32 masters, as ``DeviceReconstructor`` does.  A fold-in user
    passes ``transformer.factor(target)`` as the row factor.

    An operator is written from four pieces: ``_block`` (its rows and exclusion lists, checked), ``_workspace`` (what the
    library asks for), ``_on_device`` (H and the uploads of the call, accounted) and ``_launch`` (the one way into the
    library: it records ``peak_bytes`` and writes the operand prefix of ``_operands``)."""

    ENTRY_CHUNK = 1 << 22                # entries per skf_complete_entries call

    def __init__(self, S, G_col, dtype='f64', runtime=None):
        if G_col is None:
            raise ValueError('shape mismatch in completion')
        _ResidentFactors.__init__(self, S, G_col, dtype, runtime, 'completion')
        self._bufs = {}                  # name -> scratch Buffer, grown to the largest block seen, then reused
        self._transient = 0              # bytes of the current call's uploads (row block, exclusion lists, pairs)
        self.peak_bytes = 0              # largest device_bytes at a launch so far

    @property
    def device_bytes(self):
        """Everything this completer currently holds in HBM: the resident factors, the scratch of the largest block seen
        and the uploads of the call in flight."""
        return self.s.nbytes + self.b.nbytes + sum(b.nbytes for b in self._bufs.values()) + self._transient

    def _scratch(self, name, nbytes):
        have = self._bufs.get(name)
        if have is None or have.nbytes < nbytes:
            self._bufs[name] = have = self.rt.mem.empty(nbytes)
        return have

    def _upload(self, arrays):
        bufs = [self.rt.mem.from_host(a if a.size else np.zeros(1, dtype=a.dtype), sync=False) for a in arrays]
        self.rt.mem.synchronize()
        self._transient = sum(b.nbytes for b in bufs)
        return bufs

    def _h(self, A):
        """H = A S into the scratch (m x c_j, master type); returns its Buffer."""
        m = A.shape[0]
        (a,) = self._upload([A])
        h = self._scratch('h', max(m, 1) * self.cj * self.es)
        if m:
            _device_gemm(self.rt, self.code, a.ptr, self.ci, 1, self.s.ptr, self.cj, 1, h.ptr, self.cj, m, self.cj, self.ci)
        return h, a

    def _rows_of(self, G_row_block):
        A = np.ascontiguousarray(G_row_block, dtype=self.npd)
        if A.ndim != 2 or A.shape[1] != self.ci:
            raise ValueError('shape mismatch in completion')
        return A

    @staticmethod
    def _exclusion(exclude, m):
        """[] or ``[indptr int64, indices int32]`` of the block's exclusion lists, checked against its ``m`` rows (host work
        only: a shape error costs no upload)."""
        if exclude is None:
            return []
        xl = [np.ascontiguousarray(exclude[0], dtype=np.int64), np.ascontiguousarray(exclude[1], dtype=np.int32)]
        if xl[0].shape != (m + 1,):
            raise ValueError('exclude: indptr must have one entry per row of the block, plus one')
        return xl

    def _block(self, G_row_block, exclude):
        """``(A, m, xl)``: the block's rows in the master type, their number and its checked exclusion lists."""
        A = self._rows_of(G_row_block)
        return A, A.shape[0], self._exclusion(exclude, A.shape[0])

    def _workspace(self, op, m, *extra):
        """What ``skf_complete_<op>`` asks for as workspace for ``m`` rows (``extra``: the operator's own arguments)."""
        need = C.c_size_t()
        self.rt.call('skf_complete_%s_workspace_bytes' % op, self.code, m, self.nj, *extra, C.byref(need))
        return need.value

    def _operands(self, h, m):
        """What every operator scores: ``H`` (``m x c_j``, in the scratch ``h``) against the resident column factor."""
        return self.code, h.ptr, self.cj, m, self.b.ptr, self.cj, self.nj, self.cj

    def _launch(self, op, h, m, *args, check=True):
        """``skf_complete_<op>(operands of (h, m), *args, stream)`` -- every launch comes through here, so ``peak_bytes`` sees
        what is held at each of them.  ``check=False``: the status is returned, not raised."""
        self.peak_bytes = max(self.peak_bytes, self.device_bytes)
        rc = getattr(self.rt.lib, 'skf_complete_' + op)(*(self._operands(h, m) + args + (self.rt.mem.stream,)))
        if check:
            self.rt.check(rc)
        return rc

    def _scores(self, buf, shape):
        """The scores in ``buf`` as float64."""
        return self.rt.mem.to_host(buf, shape, self.npd).astype(np.float64)

    @contextlib.contextmanager
    def _on_device(self, A, own, xl):
        """What ``topk``, ``ranks`` and ``above`` hold on the device for one block: ``H = A S`` and the uploads of the
        method's ``own`` host arrays and of the exclusion lists ``xl``, all accounted in ``_transient`` and released on
        the way out, whatever happened.  Yields ``(h, pointers of own, excl_indptr, excl_indices)``, the last two None
        without lists."""
        h, a = self._h(A)
        held = self._transient
        bufs = []
        if own or xl:
            bufs = self._upload(list(own) + xl)
            self._transient += held
        try:
            yield h, [b.ptr for b in bufs[:len(own)]], bufs[-2].ptr if xl else None, bufs[-1].ptr if xl else None
        finally:
            del a, bufs
            self._transient = 0

    def topk(self, G_row_block, k, exclude=None, col_splits=0):
        """``(idx int32 [m, k], val float64 [m, k])``: per row of the block the ``k`` best columns, best first -- higher
        score first, equal scores by lower column, NaN never; slots no candidate fills hold ``-1`` / ``-inf``.
        ``exclude = (indptr, indices)``: CSR over the rows of THIS block (columns strictly ascending within a row) of the
        columns that are no candidates; validated on the device.  ``col_splits`` 0 lets the library choose; the result
        does not depend on it."""
        A, m, xl = self._block(G_row_block, exclude)
        k, mem = int(k), self.rt.mem
        need = self._workspace('topk', m, k, int(col_splits))
        if m == 0:
            return np.zeros((0, k), dtype=np.int32), np.zeros((0, k), dtype=np.float64)
        with self._on_device(A, [], xl) as (h, _, xp, xi):
            ws = self._scratch('ws', need)
            oi = self._scratch('idx', m * k * 4)
            ov = self._scratch('val', m * k * self.es)
            self._launch('topk', h, m, k, xp, xi, oi.ptr, k, ov.ptr, k, int(col_splits), ws.ptr, ws.nbytes)
            mem.synchronize()
            return mem.to_host(oi, (m, k), np.int32), self._scores(ov, (m, k))

    def ranks(self, G_row_block, targets, exclude=None, col_splits=0):
        """``(rank int32 [n], val float64 [n])`` for the ``n`` target pairs of the block, in list order: ``rank`` is the
        number of admissible columns of the pair's row that come before the pair's column in the order of ``topk`` -- a
        higher score, or an equal score and a lower column; NaN scores, the column itself and the row's excluded columns
        are no competitors -- i.e. the pair's 0-based position in that order, and -1 where the pair's own score is NaN;
        ``val`` is that score.  An excluded pair is still ranked.  ``targets = (indptr, indices)`` and ``exclude =
        (indptr, indices)``: CSR over the rows of THIS block (columns strictly ascending within a row), validated on the
        device.  ``col_splits`` 0 lets the library choose; the result does not depend on it.  Only the block's H, its
        lists and one rank and score per pair live in HBM."""
        A, m, xl = self._block(G_row_block, exclude)
        mem = self.rt.mem
        tgt = [np.ascontiguousarray(targets[0], dtype=np.int64), np.ascontiguousarray(targets[1], dtype=np.int32)]
        if tgt[0].shape != (m + 1,):
            raise ValueError('targets: indptr must have one entry per row of the block, plus one')
        n = int(tgt[1].size)
        need = self._workspace('ranks', m, n, int(col_splits))
        if n == 0:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64)
        with self._on_device(A, tgt, xl) as (h, (tp, ti), xp, xi):
            ws = self._scratch('ws', need)
            orank = self._scratch('rank', n * 4)
            oval = self._scratch('rank_val', n * self.es)
            self._launch('ranks', h, m, tp, ti, n, xp, xi, orank.ptr, oval.ptr, int(col_splits), ws.ptr, ws.nbytes)
            mem.synchronize()
            return mem.to_host(orank, (n,), np.int32), self._scores(oval, (n,))

    ABOVE_PER_ROW = 64                   # entries per row the first call of `above` makes room for

    def above(self, G_row_block, thr, exclude=None, col_splits=0, capacity=None, max_entries=None, count_only=False):
        """``(indptr int64 [m + 1], indices int32 [n], values float64 [n])``: canonical CSR over the rows of the block of
        every column whose score is at or above the row's threshold -- ``score >= thr`` in the SCORING type (``thr``, a
        scalar or one value per row, is cast to it first), IEEE: a NaN score or threshold selects nothing, ``-inf``
        every admissible column whose score is not NaN.  Columns ascend within a row; ``values`` are the scores, with the
        bits ``topk`` and ``ranks`` give.  ``exclude = (indptr, indices)`` as for ``topk``.  The device counts, scans and
        fills; the first call makes room for ``capacity`` entries (default: ``ABOVE_PER_ROW`` per row, or what an earlier
        block needed) and is repeated ONCE with the exact count when they do not suffice -- the arrays are the same either
        way.  ``max_entries``: a count beyond it raises ``AboveLimit`` before anything of that size is allocated.
        ``col_splits`` 0 lets the library choose; the result does not depend on it.  ``count_only=True``: the count pass and
        the scan alone (``out_indices`` NULL) -- returns ``indptr`` and nothing else, allocates no entry buffer."""
        A, m, xl = self._block(G_row_block, exclude)
        t = np.asarray(thr, dtype=np.float64)
        if t.ndim > 1 or (t.ndim == 1 and t.shape != (m,)):
            raise ValueError('thr: a scalar or one value per row of the block')
        own = [np.ascontiguousarray(np.broadcast_to(t.astype(self.npd), (m,)))]
        need = self._workspace('above', m, int(col_splits))
        if m == 0:
            if count_only:
                return np.zeros(1, dtype=np.int64)
            return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64)
        with self._on_device(A, own, xl) as (h, (bt,), xp, xi):
            return self._above_on_device(h, m, bt, xp, xi, col_splits, need, capacity, max_entries, count_only)

    def _above_on_device(self, h, m, bt, xp, xi, col_splits, ws_bytes, capacity, max_entries, count_only=False):
        """The device part of ``above`` for a block that is already there: ``h`` its H, ``bt`` the DEVICE address of its
        ``m`` thresholds in the scoring type, ``xp`` / ``xi`` those of its lists (``row_best`` hands the thresholds of the
        select over without a trip to the host)."""
        mem = self.rt.mem
        ws = self._scratch('ws', ws_bytes)
        op = self._scratch('above_ptr', (m + 1) * 8)
        found = C.c_int64(-1)
        tail = (C.byref(found), int(col_splits), ws.ptr, ws.nbytes)
        if count_only:
            self._launch('above', h, m, bt, xp, xi, 0, op.ptr, None, None, *tail)
            mem.synchronize()
            return mem.to_host(op, (m + 1,), np.int64)
        if capacity is None:
            have = self._bufs.get('above_idx')
            cap = min(m * self.nj, max(self.ABOVE_PER_ROW * m, have.nbytes // 4 if have else 0))
        else:
            cap = int(capacity)
        for attempt in (0, 1):
            oi = self._scratch('above_idx', max(cap, 1) * 4)
            ov = self._scratch('above_val', max(cap, 1) * self.es)
            rc = self._launch('above', h, m, bt, xp, xi, cap, op.ptr, oi.ptr, ov.ptr, *tail, check=False)
            mem.synchronize()
            n = found.value
            if max_entries is not None and n > max_entries:
                raise AboveLimit(n)
            if rc != nat.SKF_E_WORKSPACE or attempt or n <= cap:
                self.rt.check(rc)
                break
            cap = n                  # the count pass has said how many there are: once more, with room for them
        return mem.to_host(op, (m + 1,), np.int64), mem.to_host(oi, (n,), np.int32), self._scores(ov, (n,))

    def _wants(self, k, m):
        """``k`` -- a scalar or one value per row, integers >= 0 -- as int64 [m]."""
        w = np.asarray(k)
        if w.dtype.kind not in 'iu' or w.ndim > 1 or (w.ndim == 1 and w.shape != (m,)):
            raise ValueError('k: a non-negative integer or one per row of the block')
        w = np.ascontiguousarray(np.broadcast_to(w.astype(np.int64), (m,)))
        if m and w.min() < 0:
            raise ValueError('k: a non-negative integer or one per row of the block')
        return w

    def _row_block(self, G_row_block, k, exclude, col_splits):
        """The preamble of ``row_kth`` and ``row_best``: ``(A, m, want, xl, workspace of the select, workspace of above)``."""
        A, m, xl = self._block(G_row_block, exclude)
        want, s = self._wants(k, m), int(col_splits)
        return A, m, want, xl, self._workspace('row_kth', m, s), self._workspace('above', m, s)

    def _row_kth_on_device(self, h, m, wp, xp, xi, col_splits, ws_bytes):
        """The select of ``row_kth`` on a block that is already there (``wp``: the device address of its ``want``): returns the
        scratch Buffers ``(thr, greater, equal, cands)``, written by the stream -- nothing is read back here."""
        ws = self._scratch('ws', ws_bytes)
        thr = self._scratch('row_thr', m * self.es)
        out = [self._scratch(name, m * 8) for name in ('row_greater', 'row_equal', 'row_cands')]
        self._launch('row_kth', h, m, wp, xp, xi, thr.ptr, out[0].ptr, out[1].ptr, out[2].ptr, int(col_splits), ws.ptr, ws.nbytes)
        return [thr] + out

    def _row_kth_to_host(self, bufs, m):
        mem = self.rt.mem
        mem.synchronize()
        return (self._scores(bufs[0], (m,)),) + tuple(mem.to_host(b, (m,), np.int64) for b in bufs[1:])

    def row_kth(self, G_row_block, k, exclude=None, col_splits=0):
        """``(thr float64 [m], greater int64 [m], equal int64 [m], cands int64 [m])``: per row of the block the ``k``-th
        largest candidate score (``k``: a scalar or one value per row, any size; candidates: admissible columns whose score
        is not NaN, ``cands`` of them), the candidates above it and those equal to it -- ``greater < min(k, cands) <=
        greater + equal``, and ``above(thr)`` returns exactly ``greater + equal`` entries in the row (P4 of
        csrc/skf_complete.h).  A row with ``k == 0`` or without candidates: NaN, 0, 0.  One radix select per row, every pass
        on the device.  ``exclude`` as for ``topk``; the result does not depend on ``col_splits``."""
        A, m, want, xl, need_kth, _ = self._row_block(G_row_block, k, exclude, col_splits)
        if m == 0:
            return np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        with self._on_device(A, [want], xl) as (h, (wp,), xp, xi):
            return self._row_kth_to_host(self._row_kth_on_device(h, m, wp, xp, xi, col_splits, need_kth), m)

    def row_best(self, G_row_block, k, exclude=None, col_splits=0, max_entries=None):
        """``(indptr, indices, values, thr, greater, equal)``: the CSR of ``above`` at every row's own ``k``-th score, and what
        ``row_kth`` says of it -- per row the ``greater`` columns that beat the ``k``-th score and the ``equal`` that tie with
        it.  H is formed once and the lists are uploaded once; the thresholds of the select stay on the device and go
        straight into the count and the fill.  ``max_entries`` and the accounting in ``peak_bytes`` as for ``above``."""
        A, m, want, xl, need_kth, need_above = self._row_block(G_row_block, k, exclude, col_splits)
        if m == 0:
            return (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int64),
                    np.zeros(0, dtype=np.int64))
        with self._on_device(A, [want], xl) as (h, (wp,), xp, xi):
            self._scratch('ws', max(need_kth, need_above))
            bufs = self._row_kth_on_device(h, m, wp, xp, xi, col_splits, need_kth)
            # room for what is wanted and a tie of one more per row; a longer tie costs one more count pass
            have = self._bufs.get('above_idx')
            cap = min(m * self.nj, max(int(np.minimum(want, self.nj).sum()) + m, have.nbytes // 4 if have else 0))
            csr = self._above_on_device(h, m, bufs[0].ptr, xp, xi, col_splits, need_above, cap, max_entries)
            return csr + self._row_kth_to_host(bufs, m)[:3]

    DIGIT_PLAN = {4: (11, 11, 10), 8: (11, 11, 11, 11, 11, 9)}      # item size of the scoring type -> digit bits per pass

    def digits(self, G_row_block, prefix, prefix_bits, digit_bits, hist, exclude=None, col_splits=0):
        """One counting pass of the radix select over the block's candidates (admissible, not NaN): every candidate whose
        order-preserving key (csrc/skf_complete.h) begins with the ``prefix_bits`` bits of ``prefix`` adds one to the bin of
        its next ``digit_bits`` (at most 11) bits in ``hist``, a device buffer of ``1 << digit_bits`` uint64 words OWNED BY
        THE CALLER: it is added to, never cleared, so the blocks of one pass sum on the device.  ``exclude`` as for
        ``topk``; the counts do not depend on ``col_splits``."""
        A, m, xl = self._block(G_row_block, exclude)
        if hist.nbytes < 8 << max(int(digit_bits), 0):
            raise ValueError('hist: a device buffer of 1 << digit_bits uint64 words')
        need = self._workspace('digits', m, int(col_splits))
        with self._on_device(A, [], xl) as (h, _, xp, xi):
            ws = self._scratch('ws', need)
            self._launch('digits', h, m, xp, xi, int(prefix), int(prefix_bits), int(digit_bits), hist.ptr, int(col_splits),
                         ws.ptr, ws.nbytes)
            self.rt.mem.synchronize()

    def kth(self, blocks, n, col_splits=0):
        """``(T, n_greater, n_equal, n_candidates)``: ``T`` (float64 of the scoring type's value) is the ``n``-th largest
        candidate score over ALL the row blocks -- ``blocks()`` returns a fresh iterator of ``(G_row_block, exclude)`` and
        is called once per pass --, ``n_greater`` candidates score above it and ``n_equal`` equal it:
        ``n_greater < n <= n_greater + n_equal``, and ``above(T)`` over the same blocks returns exactly ``n_greater +
        n_equal`` entries (P3 of csrc/skf_complete.h).  Fewer than ``n`` candidates: the smallest candidate score, and
        ``n_greater + n_equal == n_candidates``; none at all: ``T`` is NaN.  A radix select: 3 passes of ``digits`` over
        the blocks in f32 (11 / 11 / 10 key bits), 6 in f64 (11 x 5 + 9); after each the 2048 counts are read back and
        ``digit_walk`` extends the prefix.  Nothing but the histogram (16 KB) is held beside a block's usual state."""
        n = int(n)
        if n < 1:
            raise ValueError('n must be at least 1')
        mem = self.rt.mem
        prefix, pbits, greater, cands, equal = 0, 0, 0, 0, 0
        for db in self.DIGIT_PLAN[self.es]:
            hist = self._bufs['hist'] = mem.from_host(np.zeros(1 << db, dtype=np.uint64))
            for G_row_block, exclude in blocks():
                self.digits(G_row_block, prefix, pbits, db, hist, exclude=exclude, col_splits=col_splits)
            counts = mem.to_host(hist, (1 << db,), np.uint64)
            if pbits == 0:
                cands = int(counts.astype(object).sum())
                if cands == 0:
                    return float('nan'), 0, 0, 0
                n = min(n, cands)
            d, above = digit_walk(counts, n - greater)
            greater += above
            equal = int(counts[d])
            prefix, pbits = (prefix << db) | d, pbits + db
        return float(score_of_key(prefix, self.npd)), greater, equal, cands

    def hist(self, G_row_block, edges, hist, exclude=None, targets=None, hist_targets=None, col_splits=0):
        """One walk of ``skf_complete_hist`` over the block: every candidate (admissible, not NaN) adds one to the bin
        ``#{t : edges[t] <= score}`` of ``hist``, and a candidate that is one of ``targets`` (``(indptr, indices)``: CSR over the
        rows of THIS block, as for ``ranks``) adds one to that bin of ``hist_targets`` as well.  ``edges`` (the scoring type,
        non-decreasing, no NaN, at most ``SKF_HIST_MAX_EDGES``), ``hist`` and ``hist_targets`` (``len(edges) + 1`` uint64 words
        each) are device buffers OWNED BY THE CALLER: the histograms are added to, never cleared, so the blocks of one walk
        sum on the device.  ``exclude`` as for ``topk``; the counts do not depend on ``col_splits``."""
        A, m, xl = self._block(G_row_block, exclude)
        n_edges = edges.nbytes // self.es
        if (targets is None) != (hist_targets is None):
            raise ValueError('targets and hist_targets come together')
        if hist.nbytes < 8 * (n_edges + 1) or (hist_targets is not None and hist_targets.nbytes < 8 * (n_edges + 1)):
            raise ValueError('hist: a device buffer of len(edges) + 1 uint64 words')
        tgt = []
        if targets is not None:
            tgt = [np.ascontiguousarray(targets[0], dtype=np.int64), np.ascontiguousarray(targets[1], dtype=np.int32)]
            if tgt[0].shape != (m + 1,):
                raise ValueError('targets: indptr must have one entry per row of the block, plus one')
        n = int(tgt[1].size) if tgt else 0
        need = self._workspace('hist', m, n, int(col_splits))
        with self._on_device(A, tgt, xl) as (h, tl, xp, xi):
            ws = self._scratch('ws', need)
            tp, ti = tl if tgt else (None, None)
            self._launch('hist', h, m, edges.ptr, n_edges, xp, xi, tp, ti, n, hist.ptr, hist_targets.ptr if tgt else None,
                         int(col_splits), ws.ptr, ws.nbytes)
            self.rt.mem.synchronize()

    def histogram(self, blocks, edges, col_splits=0):
        """``(counts int64 [len(edges) + 1], target_counts or None, n_candidates)`` over ALL the row blocks: ``counts[b]``
        candidates score in bin ``b = #{t : edges[t] <= score}`` -- the comparison is made in the scoring type, to which
        ``edges`` (a host array of ANY length >= 1, non-decreasing, no NaN) is cast -- and ``target_counts[b]`` of them are
        targets.  ``blocks()`` returns a fresh iterator of ``(G_row_block, exclude, targets_or_None)`` and is called once per
        walk; the blocks give targets all or none.  More than ``SKF_HIST_MAX_EDGES`` edges take one walk per chunk of that
        many; a chunk's counts at or above each of its edges are exact, and the bins of the whole are their differences:
        integer arithmetic, the histogram one walk over all the edges would give.  Beside a block's usual state only the
        edges of a chunk and its two histograms (at most 16 KB each) are held."""
        e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).astype(self.npd))
        if e.ndim != 1 or e.size < 1:
            raise ValueError('edges: a one-dimensional array of at least one value')
        if np.isnan(e).any() or (e[1:] < e[:-1]).any():
            raise ValueError('edges: no NaN, non-decreasing')
        mem = self.rt.mem
        at_or_above = [[], []]               # per edge, Python integers: all candidates / targets at or above it
        total, with_targets = [0, 0], None
        for c0 in range(0, e.size, nat.SKF_HIST_MAX_EDGES):
            chunk = e[c0:c0 + nat.SKF_HIST_MAX_EDGES]
            self._bufs['hist_edges'] = de = mem.from_host(chunk)
            bufs = [None, None]
            for G_row_block, exclude, targets in blocks():
                if with_targets is None:
                    with_targets = targets is not None
                if (targets is not None) != with_targets:
                    raise ValueError('histogram: the blocks give targets all or none')
                for i in range(1 + with_targets):
                    if bufs[i] is None:
                        bufs[i] = self._bufs[('hist', 'hist_targets')[i]] = mem.from_host(np.zeros(chunk.size + 1, dtype=np.uint64))
                self.hist(G_row_block, de, bufs[0], exclude=exclude, targets=targets, hist_targets=bufs[1], col_splits=col_splits)
            for i in range(2):
                if bufs[i] is None:          # no block at all, or no targets
                    got = [0] * (chunk.size + 1)
                else:
                    got = [int(v) for v in mem.to_host(bufs[i], (chunk.size + 1,), np.uint64)]
                total[i] = sum(got)
                run = 0
                tail = []
                for v in reversed(got[1:]):
                    run += v
                    tail.append(run)
                at_or_above[i].extend(reversed(tail))
        out = []
        for i in range(2):
            a = at_or_above[i]
            bins = [total[i] - a[0]] + [a[t] - a[t + 1] for t in range(len(a) - 1)] + [a[-1]]
            out.append(np.array(bins, dtype=np.int64))
        return out[0], out[1] if with_targets else None, total[0]

    def entries(self, G_row, rows, cols):
        """``float64 [n]``: ``X[rows[e], cols[e]]``.  Only the DISTINCT rows of ``G_row`` that ``rows`` names are uploaded
        (remapped); the pairs go through in chunks of ``ENTRY_CHUNK``, so ``n`` has no limit."""
        rows = np.asarray(rows).reshape(-1)
        cols = np.asarray(cols).reshape(-1)
        if rows.shape != cols.shape:
            raise ValueError('rows and cols must have the same length')
        G_row = np.asarray(G_row)
        if G_row.ndim != 2 or G_row.shape[1] != self.ci:
            raise ValueError('shape mismatch in completion')
        out = np.empty(rows.size, dtype=np.float64)
        if rows.size == 0:
            return out
        if rows.min() < 0 or rows.max() >= G_row.shape[0]:
            raise ValueError('a row index is outside the row factor')
        if cols.min() < -2 ** 31 or cols.max() >= 2 ** 31:
            raise ValueError('a column index is outside the column factor')
        used, local = np.unique(rows, return_inverse=True)
        h, a = self._h(self._rows_of(G_row[used]))
        held = self._transient
        mem = self.rt.mem
        try:
            for e0 in range(0, rows.size, self.ENTRY_CHUNK):
                sl = slice(e0, min(e0 + self.ENTRY_CHUNK, rows.size))
                n = sl.stop - sl.start
                br, bc = self._upload([local[sl].astype(np.int32), cols[sl].astype(np.int32)])
                self._transient += held
                o = self._scratch('entries', n * self.es)
                self._launch('entries', h, used.size, br.ptr, bc.ptr, n, o.ptr)
                mem.synchronize()
                out[sl] = mem.to_host(o, (n,), self.npd)
                del br, bc
        finally:
            del a
            self._transient = 0
        return out
