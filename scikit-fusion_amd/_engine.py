"""Host-side driver of one solver run: builds a plan in ``libskfusion_hip.so`` from the
``R / Theta / M`` dictionaries that arrive at the reference's functional seam
(``dfmf(**params)``, reference _dfmf.py:127; ``dfmc``, _dfmc.py:181; ``transform``,
_dfmf.py:330), keeps every matrix resident in HBM for the whole ``max_iter`` loop and copies
``G`` / ``S`` back once at the end (or per iteration when a callback is installed).
"""
import ctypes as C

import numpy as np

from . import _native as nat
# the consuming side of a fitted model has a module of its own; its names stay importable from here
from ._complete import (DeviceMatrix, DeviceReconstructor, _device_gemm, chain_backbone, device_reconstruct,      # noqa: F401
                        AboveLimit, digit_walk, score_of_key, DeviceCompleter)
# ... and so has the communicator glue of the sharded fits (the RCCL rendezvous, its cache, the torch.distributed transport)
from ._comm import (_all_reduce_sum, _exchange, _RCCL, _group_token, release_rccl_comms, comm_info,              # noqa: F401
                    _shared_rccl_comm, _torch_collective)


class PackedMask(object):
    """A DFMC mask in HBM as packed bits: bit (c & 7) of byte [r * ld + (c >> 3)], 1 = unknown entry
    (SKF_REL_MASK_BITS, include/skfusion_hip.h)."""

    def __init__(self, buf, shape, ld, known=0):
        self.buf, self.shape, self.ld = buf, tuple(shape), ld
        self.known = int(known)         # number of KNOWN entries (mask == 0); 0 = not counted


class KnownEntries(object):
    """A relation given as its KNOWN entries only, canonical CSR on the host: `indptr` (n_row + 1), `indices` (columns,
    strictly ascending within a row) and `values`; every entry not stored is unknown (SKF_REL_KNOWN_CSR).  The engine's
    own container -- the API layer builds it from a ``scipy.sparse`` matrix (``Relation(..., unstored='unknown')``).
    ``known`` is the number of entries; ``toarray`` / ``mask`` give the equivalent dense relation and completion mask.
    ``unstored='zero'``: the same container for a relation whose entries that are not stored are ZERO (what a scipy.sparse
    matrix means; SKF_REL_SPARSE_CSR, DFMF and unmasked DFMC relations): `fill` is 0, there is no mask, ``toarray`` is the
    dense relation itself.
    ``by_col=True``: the lists are compressed along the COLUMN type -- `indptr` has n_col + 1
    entries and `indices` are rows, the canonical CSC -- which is what a fold-in whose target is the relation's column type
    hands to the library (SKF_REL_FOLD_CSR: lists compressed along the target's side; with ``unstored='unknown'``
    SKF_REL_FOLD_CSR | SKF_REL_FOLD_KNOWN, the fold-in on the known entries only).  Fits take row lists.  `shape` stays the
    relation's.
    ``row_fill=a, col_fill=b`` (``unstored='zero'``, row lists only): a relation with MISSING values after its fill -- the
    entries not stored hold a_r * b_c, the stored ones their true values (SKF_REL_FILL_RANK1: the filled matrix is
    a b^T + D with D sparse on the stored pattern; the library forms d = v - a_r b_c itself).  One of the two vectors is
    all ones for every fill strategy of ``Relation``.  ``expand`` gives the dense filled matrix."""

    def __init__(self, indptr, indices, values, shape, fill=0.0, unstored='unknown', by_col=False, row_fill=None, col_fill=None):
        if unstored not in ('unknown', 'zero'):
            raise ValueError("unstored must be 'unknown' or 'zero', not %r" % (unstored,))
        if (row_fill is None) != (col_fill is None):
            raise ValueError('row_fill and col_fill come together')
        if row_fill is not None and (unstored != 'zero' or by_col):
            raise ValueError("fill vectors need unstored='zero' and lists compressed along the rows")
        self.row_fill = self.col_fill = None
        if row_fill is not None:
            self.row_fill = np.ascontiguousarray(row_fill, dtype=np.float64)
            self.col_fill = np.ascontiguousarray(col_fill, dtype=np.float64)
            if self.row_fill.shape != (int(shape[0]),) or self.col_fill.shape != (int(shape[1]),):
                raise ValueError('fill vectors of %r and %r entries for a %r relation'
                                 % (self.row_fill.shape, self.col_fill.shape, tuple(shape)))
        self.unstored = unstored
        self.by_col = bool(by_col)
        if unstored == 'zero':
            fill = 0.0
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        self.indices = np.ascontiguousarray(indices, dtype=np.int32)
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.shape = (int(shape[0]), int(shape[1]))
        self.known = int(self.indices.size)
        self.fill = float(fill)         # what the mask form holds beneath its unknown entries (read by the initialisers only)

    def row_of_entries(self):
        """The outer object of every entry: its row (by_col: its column)."""
        return np.repeat(np.arange(self.shape[1 if self.by_col else 0], dtype=np.int64), np.diff(self.indptr))

    def rows_cols(self):
        """(row, column) of every entry, in list order."""
        outer, inner = self.row_of_entries(), self.indices.astype(np.int64)
        return (inner, outer) if self.by_col else (outer, inner)

    def row_slice(self, begin, count):
        """The entries of rows [begin, begin + count) as a container of their own: slices of `indices` / `values` (views) and
        `indptr` rebased to 0 -- no dense step.  What a rank of an ownership-sharded fit hands to its plan."""
        if self.by_col or self.row_fill is not None:
            raise ValueError('lists compressed along the column type and filled relations have no row slices')
        lo, hi = int(self.indptr[begin]), int(self.indptr[begin + count])
        return KnownEntries(self.indptr[begin:begin + count + 1] - lo, self.indices[lo:hi], self.values[lo:hi],
                            (count, self.shape[1]), fill=self.fill, unstored=self.unstored)

    def expand(self):
        """The dense matrix the container stands for: the stored values on their entries, elsewhere `fill` -- or, with
        fill vectors, row_fill[r] * col_fill[c] (one factor is 1: the product is the fill value itself, bit for bit)."""
        if self.row_fill is None:
            return self.toarray()
        out = np.multiply.outer(self.row_fill, self.col_fill)
        out[self.rows_cols()] = self.values
        return out

    def toarray(self, fill=None):
        """The dense relation of the mask form: the values on the known entries, `fill` (default: self.fill) elsewhere."""
        if self.row_fill is not None and fill is None:
            return self.expand()
        out = np.full(self.shape, self.fill if fill is None else fill, dtype=np.float64)
        out[self.rows_cols()] = self.values
        return out

    def mask(self):
        """True = unknown (the DFMC convention)."""
        if self.unstored == 'zero':
            raise ValueError('a relation whose unstored entries are zero has no completion mask')
        m = np.ones(self.shape, dtype=bool)
        m[self.row_of_entries(), self.indices] = False
        return m

    def validate(self):
        """The device's checks on the host (skf_plan_set_known_entries), before anything is uploaded."""
        from .fusion.base import DataFusionError
        n_r, n_c = self.shape[::-1] if self.by_col else self.shape        # (lists, range of their indices)
        p, ix = self.indptr, self.indices
        if p.ndim != 1 or p.size != n_r + 1 or p[0] != 0 or p[-1] != ix.size or self.values.shape != ix.shape:
            raise DataFusionError('known entries: indptr must run from 0 to the %d entries over %d rows' % (ix.size, n_r))
        if (np.diff(p) < 0).any():
            raise DataFusionError('known entries: indptr is not non-decreasing')
        if ix.size and (ix.min() < 0 or ix.max() >= n_c):
            raise DataFusionError('known entries: a column index outside [0, %d)' % n_c)
        if ix.size > 1:
            first = np.zeros(ix.size, dtype=bool)                   # entries that open a row: no step to check there
            first[p[:-1][p[:-1] < ix.size]] = True
            chunk = 1 << 24                                         # (no full-size temporaries: 80 M entries at config 5)
            for c0 in range(0, ix.size - 1, chunk):
                c1 = min(c0 + chunk, ix.size - 1)
                if ((ix[c0 + 1:c1 + 1] <= ix[c0:c1]) & ~first[c0 + 1:c1 + 1]).any():
                    raise DataFusionError('known entries: columns not strictly ascending within a row (canonical CSR)')
        if self.row_fill is not None and not (np.isfinite(self.row_fill).all() and np.isfinite(self.col_fill).all()):
            raise DataFusionError('known entries: a fill vector holds a value that is not finite')


class DeviceKnownEntries(object):
    """KnownEntries uploaded ONCE in the engine's element type (upload_graph: shared by the plans of concurrent restarts)."""

    def __init__(self, indptr, indices, values, shape, known, unstored='unknown', by_col=False, row_fill=None, col_fill=None,
                 fill=0.0):
        self.indptr, self.indices, self.values = indptr, indices, values
        self.row_fill, self.col_fill = row_fill, col_fill        # device vectors in the master type (SKF_REL_FILL_RANK1) or None
        self.fill = float(fill)         # KnownEntries.fill: the constant beneath the unknown entries (the initialisers read it)
        self.shape, self.known = tuple(shape), int(known)
        self.unstored = unstored        # 'unknown': SKF_REL_KNOWN_CSR, 'zero': SKF_REL_SPARSE_CSR (fits) / SKF_REL_FOLD_CSR (fold-ins)
        self.by_col = bool(by_col)      # lists compressed along the column type (fold-ins whose target it is)


def upload_known_entries(ke, dtype, mem, fold=False):
    """KnownEntries -> DeviceKnownEntries: validated on the host first (DataFusionError before any upload); values in the
    element type of the relation data (SKF_BF16: bf16 bits, rounded as dense data is: f64 -> f32 -> bf16).  Entries whose
    unstored neighbours are zero (SKF_REL_SPARSE_CSR) go up in the master type: SKF_BF16 keeps them as f32 -- and so do
    the lists of a fold-in (`fold`: SKF_REL_FOLD_CSR, with or without SKF_REL_FOLD_KNOWN)."""
    ke.validate()
    code = nat.DTYPES[dtype] if isinstance(dtype, str) else dtype
    vals = np.ascontiguousarray(ke.values, dtype=nat.NP_DTYPE[code])
    if code == nat.SKF_BF16 and ke.unstored != 'zero' and not fold:
        vals = nat.to_bf16_bits(vals)
    keep = lambda a: mem.from_host(a if a.size else np.zeros(1, dtype=a.dtype))        # (no empty allocations)
    fills = (None, None)
    if ke.row_fill is not None:         # the fill vectors in the master type, like the values beside them
        fills = tuple(keep(np.ascontiguousarray(v, dtype=nat.NP_DTYPE[code])) for v in (ke.row_fill, ke.col_fill))
    return DeviceKnownEntries(keep(ke.indptr), keep(ke.indices), keep(vals), ke.shape, ke.known, ke.unstored, ke.by_col, *fills,
                              fill=ke.fill)


def pack_mask(mask, mem):
    """Boolean host mask -> PackedMask (1/8 of the bytes cross PCIe; the engine reads one bit per entry)."""
    m = np.asarray(mask, dtype=bool)
    if m.ndim != 2:
        raise ValueError('mask is not a matrix')
    bits = np.ascontiguousarray(np.packbits(m, axis=1, bitorder='little'))
    return PackedMask(mem.from_host(bits), m.shape, bits.shape[1], known=m.size - int(np.count_nonzero(m)))


def is_binary_matrix(arr, chunk_rows=4096):
    """True when every entry of the host matrix is 0 or 1 (SKF_REL_BINARY).  Row chunks with an early exit: no
    full-size boolean temporaries, and a real-valued relation is rejected after the first chunk."""
    a = np.asarray(arr)
    if a.ndim != 2 or a.size == 0:
        return False
    for r0 in range(0, a.shape[0], chunk_rows):
        blk = a[r0:r0 + chunk_rows]
        if not bool(((blk == 0) | (blk == 1)).all()):
            return False
    return True


def device_matrix_from_tensor(t):
    """Wrap a contiguous 2-D torch tensor that lives on the engine's device (no copy).  The engine reads it on ITS stream:
    the work that produces the tensor must be complete (torch.cuda.synchronize()) before a plan is created from it."""
    assert t.dim() == 2 and t.is_contiguous()
    return DeviceMatrix(nat.Buffer(t.data_ptr(), t.numel() * t.element_size(), t), tuple(t.shape))


def fill_uniform(shape, seed, dtype='f32', scale=1.0, shift=0.0, runtime=None):
    """Device matrix of counter-based uniforms (bit-identical to oracle hash_uniform_matrix)."""
    rt = runtime or nat.get_runtime()
    code = {'f64': nat.SKF_F64, 'f32': nat.SKF_F32, 'bf16': nat.SKF_BF16}[dtype]
    esz = {'f64': 8, 'f32': 4, 'bf16': 2}[dtype]
    buf = rt.mem.empty(shape[0] * shape[1] * esz)
    rt.call('skf_fill_uniform', code, buf.ptr, shape[0], shape[1], shape[1], int(seed),
            float(scale), float(shift), rt.mem.stream)
    return DeviceMatrix(buf, shape)


def owned_rows(dtype, n_obj, part_index, part_count, runtime=None):
    """(begin, count, chunk): the rows of a type of `n_obj` objects that part `part_index` of `part_count` owns under
    SKF_OPT_OWNED_ROWS, and the rows per part of the padded layout (skf_owned_rows: the library is the one place that
    decides the boundaries)."""
    rt = runtime or nat.get_runtime()
    code = nat.DTYPES[dtype] if isinstance(dtype, str) else dtype
    b, c, ch = C.c_int64(), C.c_int64(), C.c_int64()
    rt.call('skf_owned_rows', code, int(n_obj), int(part_index), int(part_count), C.byref(b), C.byref(c), C.byref(ch))
    return b.value, c.value, ch.value


_SMALL_LIMITS = {}


def small_graph_limits(runtime=None):
    """The library's limits for the three-launch schedule of small graphs / shared launches of restarts
    (skf_small_graph_limits), read once per runtime."""
    rt = runtime or nat.get_runtime()
    if id(rt) not in _SMALL_LIMITS:
        mr, mo, mt, ml, mc, dv = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        rt.call('skf_small_graph_limits', C.byref(mr), C.byref(mo), C.byref(mt), C.byref(ml), C.byref(mc), C.byref(dv))
        _SMALL_LIMITS[id(rt)] = dict(max_rank=mr.value, max_objects=mo.value, max_types=mt.value, max_relations=ml.value,
                                     max_constraints=mc.value, constraint_nnz_divisor=dv.value)
    return _SMALL_LIMITS[id(rt)]


def known_lists_pay(known, rows, cols, rank_row, dtype):
    """Whether a masked relation of rows x cols entries, `known` of them known, is worth keeping as lists of its known entries
    (the library's own rule for whole relations, skf_plan_create: share of known entries x rank of the row type <= 4;
    SKF_DFMC_SPARSE=0 never, =1 up to a quarter known) -- for plans with owned rows, where the caller decides for all ranks
    alike (SKF_REL_KNOWN_LISTS: the flag fixes the partial-sum convention of Q and W, so the callers take rank 0's answer,
    `_distributed.same_on_all_ranks` -- an environment that differs between ranks must not split them)."""
    import os
    mode = os.environ.get('SKF_DFMC_SPARSE')
    cells = float(rows) * float(cols)
    if mode == '0' or known <= 0 or cells <= 0 or rank_row > 1024 or known > 2000000000:      # (the library's own limits)
        return False
    share = known / cells
    return share <= 0.25 and (mode == '1' or share * rank_row <= 4.0)


def _sparse_bound(nnz, n):
    """skf_theta_desc.nnz for a constraint with `nnz` non-zeros: the count itself when the matrix is sparse enough for
    the CSR path (<= n*n / the library's divisor, 16), 0 (dense product, as the reference) otherwise or when unknown."""
    nnz = int(nnz or 0)
    return max(nnz, 1) if 0 < nnz <= (int(n) * int(n)) // small_graph_limits()['constraint_nnz_divisor'] else 0


_FILL = {'mean': 0, 'row_mean': 1, 'col_mean': 2, 'const': 3}


def fill_unknown_device(data, mask, strategy, value=0.0, dtype='f64', runtime=None):
    """Host matrix (NaN / inf / masked entries unknown) -> DeviceMatrix of the engine dtype with the unknown entries
    imputed on the device (reference Relation.filled(), fusion_graph.py:464-510).  SKF_BF16: filled in f32, then
    rounded to bf16 on the device."""
    rt = runtime or nat.get_runtime()
    code = nat.DTYPES[dtype]
    work = nat.SKF_F32 if code == nat.SKF_BF16 else code
    npd = nat.NP_DTYPE[work]
    arr = np.ascontiguousarray(data, dtype=npd)
    if arr.ndim != 2:
        raise ValueError('relation data is not a matrix')
    rows, cols = arr.shape
    buf = rt.mem.from_host(arr)
    mbuf, mld = None, 0
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask, dtype=bool).astype(np.uint8))
        if m.shape != arr.shape:
            raise ValueError('mask shape mismatch')
        mbuf, mld = rt.mem.from_host(m), cols
    need = C.c_size_t()
    rt.call('skf_fill_unknown_workspace_bytes', rows, cols, C.byref(need))
    ws = rt.mem.empty(need.value)
    rt.call('skf_fill_unknown', work, buf.ptr, cols, rows, cols, mbuf.ptr if mbuf is not None else None, mld,
            _FILL[strategy], float(value), ws.ptr, need.value, rt.mem.stream)
    if code == nat.SKF_BF16:
        out = rt.mem.empty(rows * cols * 2)
        rt.call('skf_to_bf16', out.ptr, cols, work, buf.ptr, cols, rows, cols, 0, rt.mem.stream)
        rt.mem.synchronize()
        return DeviceMatrix(out, (rows, cols))
    rt.mem.synchronize()
    return DeviceMatrix(buf, (rows, cols))


def upload_matrix(data, dtype='f64', runtime=None):
    """Host matrix -> DeviceMatrix of the engine dtype (bf16: rounded on the host, as upload_graph does)."""
    rt = runtime or nat.get_runtime()
    code = nat.DTYPES[dtype]
    arr = np.ascontiguousarray(data, dtype=nat.NP_DTYPE[code])
    if arr.ndim != 2:
        raise ValueError('relation data is not a matrix')
    up = nat.to_bf16_bits(arr) if code == nat.SKF_BF16 else arr
    return DeviceMatrix(rt.mem.from_host(up), arr.shape)


def launch_count(runtime=None):
    """Kernel launches this thread has issued through the library so far (skf_launch_count); callers take differences."""
    rt = runtime or nat.get_runtime()
    n = C.c_int64()
    rt.call('skf_launch_count', C.byref(n))
    return n.value


def split_clamps(runtime=None):
    """Split-K launches of this thread whose slice count the plan's scratch could not hold (skf_split_clamps): zero unless
    the sizing rule of skf_plan_create has fallen behind the launch-time pickers."""
    rt = runtime or nat.get_runtime()
    n = C.c_int64()
    rt.call('skf_split_clamps', C.byref(n))
    return n.value


class _RowBlock(object):
    """The row-block dict a relation may carry as its fifth element (`_distributed.partition_rows`, `owned_plan`), read once:
    every key but `n_rows` may be left out and then stands for the value here.  `binary` None: no verdict on the whole
    relation came with the block, the data decides; `entries`: 'unknown' | 'zero' for a relation given as its entries."""

    def __init__(self, block):
        self.row_begin, self.n_rows = block.get('row_begin', 0), int(block['n_rows'])
        self.absent = bool(block.get('absent', False))
        self.col_side = bool(block.get('col_side', True))
        self.masked = bool(block.get('masked', False))
        self.known_lists = bool(block.get('known_lists', False))
        self.entries = block.get('entries')
        self.binary = block.get('binary')


class DevicePlan(object):
    """One (run, device) plan: relations + constraints uploaded, workspace bound."""

    def __init__(self, obj_types, n_obj, rank, relations, thetas, variant, dtype='f64',
                 target=None, engine=None, runtime=None, part=None, stream=None, sparse_known=None, owned=False):
        """relations: list of (row_type, col_type, ndarray, mask-or-None[, block]);
        thetas: list of (type, ndarray | DeviceMatrix | KnownEntries(unstored='zero') | DeviceKnownEntries -- the last two:
        the constraint as the CSR of its stored entries, never expanded; with `owned`: the slice of the rows of the type this
        part owns, shape (count, n), indptr from 0 -- SKF_OPT_THETA_OWNED_ROWS).  `block` (row-block sharding, `_distributed.partition_rows`)
        = dict(row_begin, n_rows, absent, col_side, masked): data / mask then hold only the local rows
        (None when absent); `part` = (index, count) of this plan among the row-block plans.  With `owned`, data may be the
        KnownEntries of the local rows (shape (n_rows, n_col), indptr from 0); an absent block of such a relation says which
        kind it is with entries='unknown' | 'zero'.
        `owned`: the row blocks are the ranges of `owned_rows` (SKF_OPT_OWNED_ROWS: every rank owns the same share of the rows
        of every type; such a plan iterates through iterate_dist only).
        `sparse_known` (DFMC): None = the engine decides from the number of known entries of every masked relation
        whether to keep only those (skf_relation_desc.known_bound); False = always the completed dense copy."""
        self.rt = runtime or nat.get_runtime()
        # `stream`: (raw handle, keep-alive) of a stream of its own for this plan (concurrent restarts);
        # default: the runtime's engine stream
        self._own_stream = stream
        self.stream = stream[0] if stream is not None else self.rt.mem.stream
        self.dtype = nat.DTYPES[dtype] if isinstance(dtype, str) else dtype
        if self.dtype not in nat.NP_DTYPE:
            raise ValueError('unsupported engine dtype %r' % (dtype,))
        self.np_dtype = nat.NP_DTYPE[self.dtype]
        self.types = list(obj_types)
        self.index = {t: k for k, t in enumerate(self.types)}
        self.n_obj = [int(n_obj[t]) for t in self.types]
        self.rank = [int(rank[t]) for t in self.types]
        self.relations = relations
        self.handle = nat._P()
        self._keep, self._keep_rel = [], []
        self.owned = bool(owned)
        # (what the describing methods below read)
        self._n, self._variant, self._target, self._part, self._sparse_known = n_obj, variant, target, part, sparse_known
        mem = self.rt.mem

        tdesc = (nat.TypeDesc * len(self.types))()
        for k in range(len(self.types)):
            tdesc[k].n_obj, tdesc[k].rank = self.n_obj[k], self.rank[k]
        rdesc = (nat.RelationDesc * max(len(relations), 1))()
        self.local_rows = []                             # rows of every relation this plan holds (its block, or all of them)
        # relations with missing values kept as lists: {relation: the constant beneath its unknown entries (KnownEntries.fill),
        # or None for entries plus rank one} -- what the column-mean initialisers need beside the lists (the `_filled` entry points)
        self.rel_over_fill = {}
        csr = []                                         # (relation, DeviceKnownEntries): skf_plan_set_known_entries
        for k, rel in enumerate(relations):
            dev = self._describe_relation(k, rel, rdesc[k])
            if dev is not None:
                csr.append((k, dev))
        hdesc = (nat.ThetaDesc * max(len(thetas), 1))()
        self.theta_rows = []                             # rows of every constraint kept here (the owned rows of a slice, or all)
        theta_csr = []                                   # (constraint, DeviceKnownEntries): skf_plan_set_constraint_entries
        for k, (t, data) in enumerate(thetas):
            dev = self._describe_constraint(k, t, data, hdesc[k])
            if dev is not None:
                theta_csr.append((k, dev))
        opt = nat.Options(self.dtype, variant, self.index[target] if target is not None else -1,
                          nat.SKF_ENGINE_MFMA if engine is None else engine,
                          part[0] if part else 0, part[1] if part else 0,
                          (nat.SKF_OPT_OWNED_ROWS | (nat.SKF_OPT_THETA_OWNED_ROWS if theta_csr else 0)) if owned else 0)
        self.rt.call('skf_plan_create', len(self.types), tdesc, len(relations), rdesc, len(thetas),
                     hdesc, C.byref(opt), C.byref(self.handle))
        for k, dev in csr:
            self.rt.call('skf_plan_set_known_entries', self.handle, k, dev.indptr.ptr, dev.indices.ptr, dev.values.ptr)
            if rdesc[k].flags & nat.SKF_REL_FILL_RANK1:
                self.rt.call('skf_plan_set_relation_fill', self.handle, k, dev.row_fill.ptr, dev.col_fill.ptr, self.stream)
        for k, dev in theta_csr:
            self.rt.call('skf_plan_set_constraint_entries', self.handle, k, dev.indptr.ptr, dev.indices.ptr, dev.values.ptr)
        nbytes = C.c_size_t()
        self.rt.call('skf_plan_workspace_bytes', self.handle, C.byref(nbytes))
        self.workspace_bytes = nbytes.value
        self.ws = mem.empty(nbytes.value)
        self.rt.call('skf_plan_bind_workspace', self.handle, self.ws.ptr, nbytes.value, self.stream)
        self._scalar = mem.empty(8)

    # -- the descriptors: one method per kind of input; each returns the lists to hand over after skf_plan_create, or None --
    def _describe_relation(self, k, rel, rd):
        i, j, data, mask = rel[:4]
        blk = _RowBlock(rel[4]) if len(rel) > 4 and rel[4] is not None else None
        rd.row_type, rd.col_type = self.index[i], self.index[j]
        self.local_rows.append(blk.n_rows if blk is not None else self._n[i])
        if blk is not None and blk.absent and blk.entries:
            return self._relation_without_entries_here(rd, i, j, blk)
        if isinstance(data, (KnownEntries, DeviceKnownEntries)):
            return self._relation_entries(k, rd, i, j, data, mask, blk)
        return self._relation_dense(k, rd, i, j, data, mask, blk)

    def _check_shape(self, k, i, j, shape):
        """The one dimension check of a relation: the rows this plan holds of it, all columns."""
        rows, cols = self.local_rows[k], self._n[j]
        if tuple(shape) != (rows, cols):
            raise ValueError('relation (%s,%s) dimension mismatch: %r vs object counts (%d,%d)' % (i, j, tuple(shape), rows, cols))

    def _relation_without_entries_here(self, rd, i, j, blk):
        """Row ownership, a relation given as its entries, no row of it here: no lists, only the flags."""
        if not self.owned:
            raise ValueError('relation (%s,%s): known entries take a row block under row ownership only' % (i, j))
        rd.flags = nat.SKF_REL_ABSENT | (nat.SKF_REL_SPARSE_CSR if blk.entries == 'zero' else nat.SKF_REL_KNOWN_CSR)

    def _relation_entries(self, k, rd, i, j, data, mask, blk):
        """The known entries only (SKF_REL_KNOWN_CSR), or the stored entries of a relation that is zero elsewhere
        (SKF_REL_SPARSE_CSR; with fill vectors SKF_REL_FILL_RANK1; in a fold-in SKF_REL_FOLD_CSR, and there the known entries
        SKF_REL_FOLD_CSR | SKF_REL_FOLD_KNOWN): no dense form, no mask;
        always kept as lists.  Row ownership: the CSR of the owned rows, indptr rebased to 0, columns over the whole column
        type."""
        variant, target = self._variant, self._target
        if mask is not None or (blk is not None and not self.owned):
            raise ValueError('relation (%s,%s): known entries take no mask and no row block' % (i, j))
        self._check_shape(k, i, j, data.shape)
        if blk is not None:
            rd.row_begin, rd.n_rows = int(blk.row_begin), self.local_rows[k]
        dev = data if isinstance(data, DeviceKnownEntries) else upload_known_entries(data, self.dtype, self.rt.mem,
                                                                                     fold=variant == nat.SKF_TRANSFORM)
        self._keep_rel.append(dev)
        rd.known_bound = dev.known
        if variant == nat.SKF_TRANSFORM:
            # a fold-in: the entries compressed along the target's side -- stored over zeros, or known over unknowns
            if dev.row_fill is not None:
                raise ValueError('relation (%s,%s): a filled relation with missing values is for fits, not fold-ins' % (i, j))
            if dev.by_col != (j == target and i != target):
                raise ValueError('relation (%s,%s): a fold-in takes the lists compressed along the target %s'
                                 % (i, j, target))
            rd.flags |= nat.SKF_REL_FOLD_CSR | (0 if dev.unstored == 'zero' else nat.SKF_REL_FOLD_KNOWN)
            return dev
        if dev.by_col:
            raise ValueError('relation (%s,%s): lists compressed along the column type are for fold-ins' % (i, j))
        rd.flags |= nat.SKF_REL_SPARSE_CSR if dev.unstored == 'zero' else nat.SKF_REL_KNOWN_CSR
        if dev.unstored != 'zero':
            self.rel_over_fill[k] = float(dev.fill)
        elif dev.row_fill is not None:                  # a filled relation with missing values: entries plus rank one
            rd.flags |= nat.SKF_REL_FILL_RANK1
            self.rel_over_fill[k] = None
        return dev

    def _relation_dense(self, k, rd, i, j, data, mask, blk):
        """A dense relation, or the rows of its block: a host array (uploaded here; SKF_BF16: as bf16 bit patterns) or a
        DeviceMatrix, with its mask in any of the three forms."""
        if blk is not None:
            rd.row_begin, rd.n_rows = int(blk.row_begin), blk.n_rows
            rd.flags = ((nat.SKF_REL_ABSENT if blk.absent else 0) | (0 if blk.col_side else nat.SKF_REL_NO_COL_SIDE) |
                        (nat.SKF_REL_MASKED if blk.masked else 0) |
                        (nat.SKF_REL_KNOWN_LISTS if blk.known_lists else 0))      # (row ownership: decided for all ranks alike by the caller)
            if blk.absent:
                return None
        bf16_bitmap = self.dtype == nat.SKF_BF16 and mask is None     # a 0 / 1 relation is kept as a bitmap (1/16 of the bytes)
        if isinstance(data, DeviceMatrix):
            shape, buf, ld, binary = data.shape, data.buf, data.ld, data.binary
        else:
            arr = np.ascontiguousarray(data, dtype=self.np_dtype)
            if arr.ndim != 2:
                raise ValueError('relation %d is not a matrix' % k)
            # A row block carries the verdict on the WHOLE relation (`binary`), so that every rank of a row-sharded fit
            # takes the same contraction path for it
            binary = bf16_bitmap and (blk.binary if blk is not None and blk.binary is not None else is_binary_matrix(arr))
            # SKF_BF16: relations are handed over as bf16 bit patterns
            buf = self.rt.mem.from_host(nat.to_bf16_bits(arr) if self.dtype == nat.SKF_BF16 else arr)
            shape, ld = arr.shape, arr.shape[1]
        if binary and bf16_bitmap:
            rd.flags |= nat.SKF_REL_BINARY
        self._check_shape(k, i, j, shape)
        self._keep_rel.append(buf)
        rd.data, rd.ld = buf.ptr, ld
        if mask is not None:
            mbuf, rd.mask_ld, rd.known_bound, is_bits = self._mask_buffer(mask, shape, i, j)
            self._keep_rel.append(mbuf)
            rd.mask = mbuf.ptr
            if is_bits:
                rd.flags |= nat.SKF_REL_MASK_BITS
        if self._sparse_known is False or (blk is not None and not blk.known_lists):
            rd.known_bound = 0
        return None

    def _mask_buffer(self, mask, shape, i, j):
        """(buffer, ld, known entries, is_bits) of a mask in any of its three forms: packed bits already in HBM
        (PackedMask: upload_graph), uint8 bytes already in HBM (DeviceMatrix: device-generated data), or a host array,
        packed and uploaded here."""
        on_device = isinstance(mask, (PackedMask, DeviceMatrix))
        m = mask if on_device else pack_mask(mask, self.rt.mem)
        if tuple(m.shape) != tuple(shape):
            raise ValueError('mask shape mismatch for relation (%s,%s)' % (i, j))
        return m.buf, m.ld, m.known, not isinstance(mask, DeviceMatrix)

    def _describe_constraint(self, k, t, data, hd):
        n = self._n[t]
        self.theta_rows.append(int(n))
        hd.type = self.index[t]
        if isinstance(data, (KnownEntries, DeviceKnownEntries)):
            return self._constraint_entries(k, hd, t, n, data)
        if isinstance(data, DeviceMatrix):
            return self._constraint_device(hd, t, n, data)
        return self._constraint_host(hd, t, n, data)

    def _constraint_entries(self, k, hd, t, n, data):
        """The stored entries of a constraint that is zero elsewhere (skf_theta_desc.data == NULL): no dense form, always
        kept as lists; values in the master type.  Row ownership: the rows [begin, begin + count) this part owns, over all
        columns."""
        if data.unstored != 'zero' or data.by_col:
            raise ValueError("constraint on %s: entries need unstored='zero', compressed along the rows" % (t,))
        if self.owned:
            self.theta_rows[k] = owned_rows(self.dtype, n, self._part[0], self._part[1], self.rt)[1]
        if tuple(data.shape) != (self.theta_rows[k], n):
            raise ValueError('constraint on %s dimension mismatch: %r vs (%d,%d)' % (t, tuple(data.shape), self.theta_rows[k], n))
        dev = data if isinstance(data, DeviceKnownEntries) else upload_known_entries(data, self.dtype, self.rt.mem)
        self._keep.append(dev)
        hd.data, hd.ld, hd.nnz = None, 0, dev.known
        return dev

    def _constraint_device(self, hd, t, n, data):
        """A dense constraint already in HBM, master dtype; `nnz` as its maker counted it (0: nobody did)."""
        if tuple(data.shape) != (n, n):
            raise ValueError('constraint on %s dimension mismatch' % (t,))
        self._keep.append(data.buf)
        hd.data, hd.ld, hd.nnz = data.buf.ptr, data.ld, _sparse_bound(getattr(data, 'nnz', 0), n)

    def _constraint_host(self, hd, t, n, data):
        """A dense constraint on the host.  A sparse one (lambda I, a few must-link pairs per object, dicty's ppi) is kept
        as CSR on the device: `nnz` says so."""
        arr = np.ascontiguousarray(data, dtype=self.np_dtype)
        if arr.shape != (n, n):
            raise ValueError('constraint on %s dimension mismatch' % (t,))
        buf = self.rt.mem.from_host(arr)
        self._keep.append(buf)
        hd.data, hd.ld, hd.nnz = buf.ptr, arr.shape[1], _sparse_bound(int(np.count_nonzero(arr)), n)

    def release_relation_data(self):
        """SKF_BF16: the relations (and every engine's masks) were copied into the engine's own layout at
        bind time; the caller's buffers are not referenced afterwards and may be dropped.  The f32 / f64
        engines keep reading unmasked relations in place: no-op for them."""
        if self.dtype == nat.SKF_BF16:
            self._keep_rel = []

    # -- factors ---------------------------------------------------------------------------
    def set_factor(self, t, G):
        k = self.index[t]
        if isinstance(G, DeviceMatrix):
            if G.shape != (self.n_obj[k], self.rank[k]):
                raise ValueError('factor of %s has shape %r' % (t, G.shape))
            self.rt.call('skf_set_factor', self.handle, k, G.buf.ptr, G.ld, self.stream)
            self.rt.mem.synchronize()
            return
        arr = np.ascontiguousarray(G, dtype=self.np_dtype)
        if arr.shape != (self.n_obj[k], self.rank[k]):
            raise ValueError('factor of %s has shape %r, expected %r'
                             % (t, arr.shape, (self.n_obj[k], self.rank[k])))
        buf = self.rt.mem.from_host(arr)
        self.rt.call('skf_set_factor', self.handle, k, buf.ptr, arr.shape[1], self.stream)
        self.rt.mem.synchronize()

    def set_factors(self, G, sync=True):
        """Every factor of {type: array} (or {(type, type): array}) with ONE device synchronisation instead of two per
        factor -- on small graphs the synchronisations of set-up and read-back cost as much as the iterations.
        sync=False: the caller synchronises before the plan is iterated (several plans set up together)."""
        keep = []
        for key, arr in G.items():
            t = key[0] if isinstance(key, tuple) else key
            k = self.index[t]
            arr = np.ascontiguousarray(arr, dtype=self.np_dtype)
            if arr.shape != (self.n_obj[k], self.rank[k]):
                raise ValueError('factor of %s has shape %r, expected %r' % (t, arr.shape, (self.n_obj[k], self.rank[k])))
            keep.append((k, self.rt.mem.from_host(arr, sync=False), arr.shape[1]))
        self.rt.mem.synchronize()                       # the uploads (torch's stream) before the engine's copies
        for k, buf, ld in keep:
            self.rt.call('skf_set_factor', self.handle, k, buf.ptr, ld, self.stream)
        self._pending_uploads = keep                    # alive until the copies have run
        if sync:
            self.rt.mem.synchronize()
            self._pending_uploads = None

    # -- the column-mean initialisers on the device (csrc/skf_init.h; reference _init.py:20-61) -----------
    def relation_norms(self, rel, fill=None):
        """(row_sq, col_sq): the float64 sums of SQUARES of every row and every column of relation `rel` as the plan
        stores it (skf_plan_relation_norms) -- what `random_c` ranks the columns of the relation's two views by.  Exact for
        data whose squares add up exactly; the same bits on every run.  SkfNativeError (SKF_E_INVALID) for a relation the
        plan does not hold whole and unmasked.  A relation with missing values kept as lists -- its known entries over the
        constant the plan remembers (KnownEntries.fill; `fill` overrides it, and names it for lists the plan built from a
        mask), or entries plus rank one -- goes through skf_plan_relation_norms_filled: every line of the FILLED relation."""
        i, j = self.relations[rel][0], self.relations[rel][1]
        ni, nj = self.n_obj[self.index[i]], self.n_obj[self.index[j]]
        mem = self.rt.mem
        need = C.c_size_t()
        filled = fill is not None or rel in self.rel_over_fill
        if fill is None:
            fill = self.rel_over_fill.get(rel) or 0.0
        self.rt.call('skf_plan_relation_norms_filled_workspace_bytes' if filled else 'skf_plan_relation_norms_workspace_bytes',
                     self.handle, rel, C.byref(need))
        ws = mem.empty(max(need.value, 1))
        rs, cs = mem.empty(max(ni, 1) * 8), mem.empty(max(nj, 1) * 8)
        if filled:
            self.rt.call('skf_plan_relation_norms_filled', self.handle, rel, float(fill), rs.ptr, cs.ptr, ws.ptr, need.value, self.stream)
        else:
            self.rt.call('skf_plan_relation_norms', self.handle, rel, rs.ptr, cs.ptr, ws.ptr, need.value, self.stream)
        mem.synchronize()
        return mem.to_host(rs, (ni,), np.float64), mem.to_host(cs, (nj,), np.float64)

    def init_column_means(self, t, views, sync=True):
        """The factor of type `t` <- 1e-5 + sum over `views` of |mean of the chosen columns| (skf_plan_init_column_means,
        then skf_set_factor): `views` = [(relation index, sel)] in the order the reference walks the relations of `t`, sel an
        integer array c x take whose row k names the columns -- of the relation when `t` is its row type, of its transpose
        when `t` is its column type -- averaged into factor column k.  The indices of a row must be distinct (checked here:
        ValueError); their range is checked on the device (SkfNativeError, SKF_E_INVALID, nothing written).
        A view may be (relation index, sel, fill): the constant beneath the unknown entries of a known-entry relation, where
        the plan does not remember it (lists built from a mask) or to override it.  When a view is a relation with missing
        values kept as lists, the call goes through skf_plan_init_column_means_filled (all views of the type in one call).
        sync=False: the caller synchronises before the plan is iterated."""
        k = self.index[t]
        n, c = self.n_obj[k], self.rank[k]
        mem = self.rt.mem
        desc = (nat.InitView * max(len(views), 1))()
        fills = (C.c_double * max(len(views), 1))()
        filled = False
        keep = []
        for v, view in enumerate(views):
            rel, sel = view[0], view[1]
            fill = view[2] if len(view) > 2 else None
            filled = filled or fill is not None or rel in self.rel_over_fill
            fills[v] = float(fill if fill is not None else (self.rel_over_fill.get(rel) or 0.0))
            s = np.ascontiguousarray(sel, dtype=np.int32)
            if s.ndim != 2 or s.shape[0] != c:
                raise ValueError('view %d of %s: the selection has shape %r, expected (%d, take)' % (v, t, s.shape, c))
            if s.shape[1] > 1:
                ordered = np.sort(s, axis=1)
                if (ordered[:, 1:] == ordered[:, :-1]).any():
                    raise ValueError('view %d of %s: a column is chosen twice for one factor column' % (v, t))
            buf = mem.from_host(s if s.size else np.zeros(1, dtype=np.int32), sync=False)
            keep.append(buf)
            desc[v].rel, desc[v].take, desc[v].sel = int(rel), int(s.shape[1]), buf.ptr
        mem.synchronize()                               # the uploads (torch's stream) before the engine's launches
        need = C.c_size_t()
        self.rt.call('skf_plan_init_column_means_filled_workspace_bytes' if filled else 'skf_plan_init_column_means_workspace_bytes',
                     self.handle, k, len(views), desc, C.byref(need))
        ws = mem.empty(need.value)
        g0 = mem.empty(max(n * c, 1) * np.dtype(self.np_dtype).itemsize)
        if filled:
            self.rt.call('skf_plan_init_column_means_filled', self.handle, k, len(views), desc, fills, g0.ptr, c, ws.ptr, need.value,
                         self.stream)
        else:
            self.rt.call('skf_plan_init_column_means', self.handle, k, len(views), desc, g0.ptr, c, ws.ptr, need.value, self.stream)
        self.rt.call('skf_set_factor', self.handle, k, g0.ptr, c, self.stream)
        keep += [ws, g0]
        self._pending_init = getattr(self, '_pending_init', None) or []
        self._pending_init.append(keep)                 # alive until the launches have run
        if sync:
            mem.synchronize()
            self._pending_init = None

    def fetch_results(self, types, n_rel):
        """Issues the copies of every factor of `types` and the first `n_rel` backbones into device buffers; the caller
        synchronises once (for any number of plans) and calls read_results."""
        out = []
        for t in types:
            k = self.index[t]
            shape = (self.n_obj[k], self.rank[k])
            buf = self.rt.mem.empty(shape[0] * shape[1] * np.dtype(self.np_dtype).itemsize)
            self.rt.call('skf_get_factor', self.handle, k, buf.ptr, shape[1], self.stream)
            out.append((buf, shape))
        for rel in range(n_rel):
            shape = self._backbone_shape(rel)
            buf = self.rt.mem.empty(shape[0] * shape[1] * np.dtype(self.np_dtype).itemsize)
            self.rt.call('skf_get_backbone', self.handle, rel, buf.ptr, shape[1], self.stream)
            out.append((buf, shape))
        return out

    def read_results(self, fetched):
        return [self.rt.mem.to_host(buf, shape, self.np_dtype).astype(np.float64) for buf, shape in fetched]

    def get_factor(self, t):
        k = self.index[t]
        shape = (self.n_obj[k], self.rank[k])
        buf = self.rt.mem.empty(shape[0] * shape[1] * np.dtype(self.np_dtype).itemsize)
        self.rt.call('skf_get_factor', self.handle, k, buf.ptr, shape[1], self.stream)
        self.rt.mem.synchronize()
        return self.rt.mem.to_host(buf, shape, self.np_dtype).astype(np.float64)

    def _backbone_shape(self, rel):
        i, j = self.relations[rel][0], self.relations[rel][1]
        return (self.rank[self.index[i]], self.rank[self.index[j]])

    def set_backbone(self, rel, S):
        shape = self._backbone_shape(rel)
        arr = np.ascontiguousarray(S, dtype=self.np_dtype)
        if arr.shape != shape:
            raise ValueError('backbone %d has shape %r, expected %r' % (rel, arr.shape, shape))
        buf = self.rt.mem.from_host(arr)
        self.rt.call('skf_set_backbone', self.handle, rel, buf.ptr, shape[1], self.stream)
        self.rt.mem.synchronize()

    def get_backbone(self, rel):
        shape = self._backbone_shape(rel)
        buf = self.rt.mem.empty(shape[0] * shape[1] * np.dtype(self.np_dtype).itemsize)
        self.rt.call('skf_get_backbone', self.handle, rel, buf.ptr, shape[1], self.stream)
        self.rt.mem.synchronize()
        return self.rt.mem.to_host(buf, shape, self.np_dtype).astype(np.float64)

    def get_contraction(self, rel, which, rows=None):
        """P = R G_j (which=0) or Q = R^T G_i (which=1) as the last iteration left it (verification accessor); a masked
        relation kept as lists of its known entries answers which=2 with the row-side product P S^T instead of P."""
        i, j = self.relations[rel][0], self.relations[rel][1]
        if which == 0:
            shape = (rows if rows is not None else self.n_obj[self.index[i]], self.rank[self.index[j]])
        elif which == 2:
            shape = (rows if rows is not None else self.n_obj[self.index[i]], self.rank[self.index[i]])
        else:
            shape = (self.n_obj[self.index[j]], self.rank[self.index[i]])
        buf = self.rt.mem.empty(shape[0] * shape[1] * np.dtype(self.np_dtype).itemsize)
        self.rt.call('skf_get_contraction', self.handle, rel, which, buf.ptr, shape[1], self.stream)
        self.rt.mem.synchronize()
        return self.rt.mem.to_host(buf, shape, self.np_dtype)

    def relation_lists(self, rel, by_col=False):
        """(indptr, indices, values) of the entry lists relation `rel` keeps (verification accessor): the row lists, or with
        by_col the column lists -- canonical CSR / CSC whatever the number of parts the engine cut them into.  A filled
        relation with missing values (fill vectors, SKF_REL_FILL_RANK1): the values are d = v - a_r b_c, what the passes
        multiply, not the stored values."""
        j = self.relations[rel][1]
        n_out = self.n_obj[self.index[j]] if by_col else self.local_rows[rel]      # (row ownership: local rows, local indices)
        parts, nnz = C.c_int32(), C.c_int64()
        self.rt.call('skf_get_relation_lists', self.handle, rel, int(bool(by_col)), C.byref(parts), C.byref(nnz), None, None,
                     None, self.stream)
        mem, item = self.rt.mem, np.dtype(self.np_dtype).itemsize
        bp = mem.empty((n_out * parts.value + 1) * 8)
        bi, bv = mem.empty(max(nnz.value, 1) * 4), mem.empty(max(nnz.value, 1) * item)
        self.rt.call('skf_get_relation_lists', self.handle, rel, int(bool(by_col)), None, None, bp.ptr, bi.ptr, bv.ptr,
                     self.stream)
        mem.synchronize()
        ptr = mem.to_host(bp, (n_out * parts.value + 1,), np.int64)[::parts.value].copy()
        return (ptr, mem.to_host(bi, (max(nnz.value, 1),), np.int32)[:nnz.value].copy(),
                mem.to_host(bv, (max(nnz.value, 1),), self.np_dtype)[:nnz.value].copy())

    def constraint_lists(self, k):
        """(indptr, indices, values) of the lists constraint `k` keeps (verification accessor): one handed over dense and
        compacted, one given as its entries, or -- row ownership -- the slice of the owned rows (indptr of count + 1 pointers
        from 0, global columns).  SkfNativeError (SKF_E_INVALID) for a constraint kept dense."""
        rows, nnz = C.c_int64(), C.c_int64()
        self.rt.call('skf_get_constraint_lists', self.handle, k, C.byref(rows), C.byref(nnz), None, None, None, self.stream)
        mem, item = self.rt.mem, np.dtype(self.np_dtype).itemsize
        bp = mem.empty((rows.value + 1) * 8)
        bi, bv = mem.empty(max(nnz.value, 1) * 4), mem.empty(max(nnz.value, 1) * item)
        self.rt.call('skf_get_constraint_lists', self.handle, k, None, None, bp.ptr, bi.ptr, bv.ptr, self.stream)
        mem.synchronize()
        return (mem.to_host(bp, (rows.value + 1,), np.int64).copy(),
                mem.to_host(bi, (max(nnz.value, 1),), np.int32)[:nnz.value].copy(),
                mem.to_host(bv, (max(nnz.value, 1),), self.np_dtype)[:nnz.value].copy())

    def set_graph(self, enable=True):
        """Replay one captured hipGraph per iteration (concurrent restarts: include/skfusion_hip.h)."""
        self.rt.call('skf_plan_set_graph', self.handle, 1 if enable else 0)

    # -- the loop --------------------------------------------------------------------------
    def iterate(self, n_iters=1):
        self.rt.call('skf_iterate', self.handle, int(n_iters), self.stream)

    def batchable(self):
        """True when this plan can be one of the plans of iterate_batch (the schedule for small graphs)."""
        yes = C.c_int32(0)
        self.rt.call('skf_plan_batchable', self.handle, C.byref(yes))
        return bool(yes.value)

    @staticmethod
    def iterate_batch(plans, n_iters=1):
        """`n_iters` iterations of several plans of ONE graph at once (skf_iterate_batch: independent restarts of a small
        graph, every launch serving all of them) on the stream of the first plan.  Returns False, with nothing launched,
        when the plans do not batch (not the small-graph schedule, different graphs / engines): iterate them one by
        one."""
        plans = list(plans)
        first = plans[0]
        arr = (nat._P * len(plans))(*[p.handle for p in plans])
        try:
            first.rt.call('skf_iterate_batch', arr, len(plans), int(n_iters), first.stream)
        except nat.SkfNativeError as exc:
            if exc.code == nat.SKF_E_STATE:
                return False
            raise
        return True

    def synchronize(self):
        self.rt.mem.synchronize()

    # -- collectives behind the C ABI -----------------------------------------------------
    def attach_comm(self, force_callback=False):
        """Give the plan a communicator over the ranks of the torch.distributed process group, so that
        `skf_iterate_dist` issues the exchanges of a sharded iteration itself: RCCL bound by the library (backend nccl:
        torch.distributed only carries the 128-byte unique id from rank 0 to the others; ONE communicator per process,
        shared by all plans and restarts), or -- gloo groups (CPU tests, two ranks sharing one GPU in smoke runs),
        `force_callback`, or an RCCL that cannot be bound on EVERY rank -- a callback that runs the collective through
        torch.distributed on a view of the workspace.  Returns True when a communicator is attached."""
        import os
        try:
            import torch.distributed as dist
        except ImportError:
            return False
        if not (dist.is_available() and dist.is_initialized()):
            return False
        rank, world = dist.get_rank(), dist.get_world_size()
        if world <= 1 and not os.environ.get('SKF_FORCE_COLLECTIVES'):
            return False
        on_gpu = self.rt.name == 'hip'
        comm = None
        if dist.get_backend() != 'gloo' and on_gpu and not force_callback:
            comm = _shared_rccl_comm(self.rt, dist)
        if comm is not None:
            self._comm, self._comm_shared = comm, True
        else:
            self._comm = nat._P()
            self._comm_shared = False
            self._comm_fn = nat.COLLECTIVE_FN(_torch_collective(self.rt.mem, self.ws, dist, rank, world))   # keep the trampoline alive
            self.rt.call('skf_comm_create_callback', rank, world, C.cast(self._comm_fn, C.c_void_p), None, C.byref(self._comm))
        self.rt.call('skf_plan_set_comm', self.handle, self._comm)
        return True

    def comm_info(self):
        """What the attached communicator is (`_engine.comm_info`), None without one."""
        return comm_info(self.rt, self._comm) if getattr(self, '_comm', None) else None

    def attach_single_comm(self):
        """A genuine communicator of ONE rank without a transport (skf_comm_create(NULL, 0, 1)): every collective returns at
        once and the iteration is the real one -- what a fit sharded by ownership runs on when the process has no group."""
        self._comm = nat._P()
        self._comm_shared = False
        self.rt.call('skf_comm_create', None, 0, 1, C.byref(self._comm))
        self.rt.call('skf_plan_set_comm', self.handle, self._comm)

    def attach_null_comm(self, rank, world):
        """A communicator whose collectives do nothing: times the compute of rank `rank` of `world` of a sharded fit on one
        GPU (bench.py --emulate-rank); results are meaningless: the factors are never updated.  NOT for fits -- a single
        process takes attach_single_comm."""
        self._comm = nat._P()
        self._comm_shared = False
        self.rt.call('skf_comm_create_null', int(rank), int(world), C.byref(self._comm))
        self.rt.call('skf_plan_set_comm', self.handle, self._comm)

    def attach_callback_comm(self, rank, world, collective):
        """A communicator whose collectives are `collective(op, view, count, rank, world)` on tensor views of the workspace
        (in-process groups of plans: tests, tests/helpers.ThreadGroup)."""
        mem, ws = self.rt.mem, self.ws

        def trampoline(user, op, buf, count, dtype, stream):
            try:
                if dtype == nat.SKF_BF16:       # bf16 rows travel as bytes (all-gather only)
                    npd, count = np.uint8, count * 2
                else:
                    npd = nat.NP_DTYPE[dtype]
                n = count * (1 if op == 0 else world)
                view = mem.as_tensor(ws, int(buf) - ws.ptr, n * np.dtype(npd).itemsize, npd)
                collective(op, view, count, rank, world)
                return 0
            except Exception:                 # never unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        self._comm = nat._P()
        self._comm_shared = False
        self._comm_fn = nat.COLLECTIVE_FN(trampoline)
        self.rt.call('skf_comm_create_callback', int(rank), int(world), C.cast(self._comm_fn, C.c_void_p), None, C.byref(self._comm))
        self.rt.call('skf_plan_set_comm', self.handle, self._comm)

    def exchange_bytes(self, world):
        """Bytes one rank sends per iteration of the distributed iteration on a ring of `world` ranks."""
        b = C.c_size_t()
        self.rt.call('skf_exchange_bytes', self.handle, int(world), C.byref(b))
        return b.value

    def iterate_dist(self, n_iters=1):
        """Iterations of a sharded fit (whole relations or row blocks) with the exchanges issued by the library
        (include/skfusion_hip.h, skf_iterate_dist): all-reduce of W / Q, reduce-scatter of E and D, update of the owned
        range of G, all-gather of G."""
        self.rt.call('skf_iterate_dist', self.handle, int(n_iters), self.stream)

    def iterate_sharded(self, n_iters=1):
        """Iterations of a relation-sharded run: this plan holds only this rank's relations;
        the E / D accumulators are summed over the ranks before the replicated G update -- by the library's own
        collectives when a communicator is attached (attach_comm), else by one all-reduce per iteration through
        torch.distributed."""
        if getattr(self, '_comm', None):
            return self.iterate_dist(n_iters)
        off, nbytes = C.c_size_t(), C.c_size_t()
        self.rt.call('skf_accumulator_range', self.handle, C.byref(off), C.byref(nbytes))
        acc = self.rt.mem.as_tensor(self.ws, off.value, nbytes.value, self.np_dtype)
        for _ in range(int(n_iters)):
            self.rt.call('skf_accumulate', self.handle, self.stream)
            _exchange(self.rt.mem, [acc])
            self.rt.call('skf_apply_update', self.handle, self.stream)

    def _exchange_views(self):
        """Zero-copy tensor views of the four exchange ranges (None when empty)."""
        views = []
        for which in (nat.SKF_X_W, nat.SKF_X_Q, nat.SKF_X_QM, nat.SKF_X_ED):
            off, nbytes, dt = C.c_size_t(), C.c_size_t(), C.c_int32()
            self.rt.call('skf_exchange_range', self.handle, which, C.byref(off), C.byref(nbytes), C.byref(dt))
            views.append(self.rt.mem.as_tensor(self.ws, off.value, nbytes.value, nat.NP_DTYPE[dt.value])
                         if nbytes.value else None)
        return views

    def stage(self, which):
        self.rt.call('skf_stage', self.handle, int(which), self.stream)

    def iterate_rows(self, n_iters=1, reduce=None):
        """Iterations of a row-block-sharded run (every rank lists all relations, each with its row
        block): four stages with an all-reduce(sum) of W and Q, of the masked relations' Q (DFMC),
        and of E / D between them -- include/skfusion_hip.h `skf_stage`.  `reduce(tensor)` defaults
        to torch.distributed.all_reduce (RCCL on GPUs, gloo in the CPU tests); with a communicator attached
        (attach_comm) and no `reduce` the library issues the exchanges itself (skf_iterate_dist)."""
        if reduce is None and getattr(self, '_comm', None):
            return self.iterate_dist(n_iters)
        xw, xq, xqm, xed = self._exchange_views()
        mem, call, h = self.rt.mem, self.rt.call, self.handle

        def exchange(*tensors):
            _exchange(mem, tensors, reduce)
        for _ in range(int(n_iters)):
            call('skf_stage', h, nat.SKF_STAGE_CONTRACT, self.stream)
            exchange(xw, xq)
            call('skf_stage', h, nat.SKF_STAGE_BACKBONE, self.stream)
            if xqm is not None:
                exchange(xqm)
            call('skf_stage', h, nat.SKF_STAGE_ACCUMULATE, self.stream)
            exchange(xed)
            call('skf_stage', h, nat.SKF_STAGE_UPDATE, self.stream)

    def relation_sqerr(self, rel):
        """sum (R - G_i S G_j^T)^2 for relation index `rel` (device reduction, one f64 D2H)."""
        self.rt.call('skf_relation_sqerr', self.handle, rel, self._scalar.ptr, self.stream)
        self.rt.mem.synchronize()
        return float(self.rt.mem.to_host(self._scalar, (1,), np.float64)[0])

    # -- held-out pairs scored inside the fit (csrc/skf_heldout.h; include/skfusion_hip.h, skf_plan_set_heldout) ----------
    def set_heldout(self, lists, patience=0, min_delta=0.0, capacity=0):
        """Attach held-out lists: `lists` = [(relation index, rows, cols, values)] -- COO of held-out pairs with their true
        values, at most one list per relation, any order (sorted by row here, stably).  From now on every iteration of
        `iterate` scores them, judges the pooled squared error on the device (an improvement is total < best - min_delta;
        `patience` > 0: that many iterations in a row without one stop the monitor) and keeps a device copy of the best
        (G, S); `capacity`: iterations of history kept.  An empty `lists` detaches.  The lists are validated on the device:
        SkfNativeError (SKF_E_INVALID) for an index out of range or a value that is not finite, plan left unmonitored."""
        mem = self.rt.mem
        self._heldout = None
        if not lists:
            self.rt.call('skf_plan_set_heldout', self.handle, 0, None, 0, 0.0, 0, None, 0, self.stream)
            return
        desc = (nat.HeldoutDesc * len(lists))()
        keep = []
        for l, (rel, rows, cols, vals) in enumerate(lists):
            rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
            cols = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
            vals = np.ascontiguousarray(vals, dtype=self.np_dtype).reshape(-1)
            if not (rows.size == cols.size == vals.size):
                raise ValueError('held-out list of relation %d: rows, cols and values differ in length' % rel)
            for a in (rows, cols):          # (what does not fit an int32 is out of range anyway: the device refuses -1)
                a[(a < 0) | (a > 0x7fffffff)] = -1
            order = np.argsort(rows, kind='stable')
            bufs = [mem.from_host(a if a.size else np.zeros(1, dtype=a.dtype), sync=False)
                    for a in (rows[order].astype(np.int32), cols[order].astype(np.int32), vals[order])]
            keep.append(bufs)
            desc[l].rel, desc[l].n = int(rel), int(rows.size)
            desc[l].rows, desc[l].cols, desc[l].values = bufs[0].ptr, bufs[1].ptr, bufs[2].ptr
        mem.synchronize()                               # the uploads (torch's stream) before the engine's check
        need = C.c_size_t()
        self.rt.call('skf_plan_heldout_workspace_bytes', self.handle, len(lists), desc, int(capacity), C.byref(need))
        ws = mem.empty(need.value)
        self.rt.call('skf_plan_set_heldout', self.handle, len(lists), desc, int(patience), float(min_delta), int(capacity),
                     ws.ptr, need.value, self.stream)
        self._heldout = dict(keep=keep, ws=ws, n_lists=len(lists), rels=[int(x[0]) for x in lists], capacity=int(capacity), out=mem.empty(8 * len(lists)))

    def _monitored(self):
        h = getattr(self, '_heldout', None)
        if h is None:
            raise ValueError('no held-out lists attached (set_heldout)')
        return h

    def heldout_sqerr(self):
        """float64 array, one per attached list: sum (v - x)^2 over the list under the current (G, S) (skf_plan_heldout_sqerr)."""
        h = self._monitored()
        self.rt.call('skf_plan_heldout_sqerr', self.handle, h['out'].ptr, self.stream)
        self.rt.mem.synchronize()
        return self.rt.mem.to_host(h['out'], (h['n_lists'],), np.float64)

    def heldout_product(self, l):
        """H = G_i S of list `l` as the last evaluation left it (verification accessor), in the master type."""
        h = self._monitored()
        i, j = self.relations[h['rels'][l]][:2]
        shape = (self.n_obj[self.index[i]], self.rank[self.index[j]])
        buf = self.rt.mem.empty(shape[0] * shape[1] * np.dtype(self.np_dtype).itemsize)
        self.rt.call('skf_plan_get_heldout_product', self.handle, int(l), buf.ptr, shape[1], self.stream)
        self.rt.mem.synchronize()
        return self.rt.mem.to_host(buf, shape, self.np_dtype)

    def monitor(self, history=True):
        """The monitor's words (one synchronisation): dict(seen, best_iter -- 1-based, 0: none yet --, stop_iter, stopped, best,
        history -- the judged iterations x lists kept so far, or None when not asked for)."""
        h = self._monitored()
        seen, best_iter, stop_iter = C.c_int64(), C.c_int64(), C.c_int64()
        stopped, best = C.c_int32(), C.c_double()
        cap = h['capacity'] if history else 0
        host = np.zeros((max(cap, 1), h['n_lists']), dtype=np.float64)
        self.rt.call('skf_plan_get_monitor', self.handle, C.byref(seen), C.byref(best_iter), C.byref(stop_iter), C.byref(stopped),
                     C.byref(best), host.ctypes.data if cap else None, cap, self.stream)
        return dict(seen=seen.value, best_iter=best_iter.value, stop_iter=stop_iter.value, stopped=bool(stopped.value),
                    best=best.value, history=host[:min(seen.value, cap)].copy() if history else None)

    def best_factor(self, t):
        """The factor of type `t` of the best iterate (skf_get_best_factor); SkfNativeError (SKF_E_STATE) before there is one."""
        k = self.index[t]
        shape = (self.n_obj[k], self.rank[k])
        buf = self.rt.mem.empty(shape[0] * shape[1] * np.dtype(self.np_dtype).itemsize)
        self.rt.call('skf_get_best_factor', self.handle, k, buf.ptr, shape[1], self.stream)
        self.rt.mem.synchronize()
        return self.rt.mem.to_host(buf, shape, self.np_dtype).astype(np.float64)

    def best_backbone(self, rel):
        """The backbone of relation `rel` of the best iterate (skf_get_best_backbone)."""
        shape = self._backbone_shape(rel)
        buf = self.rt.mem.empty(shape[0] * shape[1] * np.dtype(self.np_dtype).itemsize)
        self.rt.call('skf_get_best_backbone', self.handle, rel, buf.ptr, shape[1], self.stream)
        self.rt.mem.synchronize()
        return self.rt.mem.to_host(buf, shape, self.np_dtype).astype(np.float64)

    def set_profiling(self, enable=True):
        self.rt.call('skf_plan_set_profiling', self.handle, 1 if enable else 0)

    def get_profile(self):
        """(total ms, launches, executed flops, relation bytes read as stored) of the launches that walk a relation
        since the last call."""
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        self.rt.call('skf_plan_get_profile', self.handle, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by))
        return ms.value, n.value, fl.value, by.value

    def close(self):
        if self.handle:
            self.rt.lib.skf_plan_destroy(self.handle)
            self.handle = nat._P()
        if getattr(self, '_comm', None):
            if not getattr(self, '_comm_shared', False):
                self.rt.lib.skf_comm_destroy(self._comm)
            self._comm = None
        self._keep, self._keep_rel = [], []
        self.ws = None
        self._heldout = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def upload_graph(rel_list, theta_list, dtype, runtime=None, fold=False):
    """Relations / masks / constraints to HBM ONCE, as DeviceMatrix entries that any number of plans can
    share (concurrent restarts of one graph): same conversions as DevicePlan applies to host arrays.  `fold`: the graph of a
    fold-in (SKF_TRANSFORM plans), whose entry lists go up in the master type."""
    rt = runtime or nat.get_runtime()
    code = nat.DTYPES[dtype] if isinstance(dtype, str) else dtype
    npd = nat.NP_DTYPE[code]
    rels, thetas = [], []
    for rel in rel_list:
        i, j, data, mask = rel[:4]
        if isinstance(data, KnownEntries):
            rels.append((i, j, upload_known_entries(data, code, rt.mem, fold=fold), mask) + tuple(rel[4:]))
            continue
        if not isinstance(data, (DeviceMatrix, DeviceKnownEntries)):
            arr = np.ascontiguousarray(data, dtype=npd)
            up = nat.to_bf16_bits(arr) if code == nat.SKF_BF16 else arr
            binary = code == nat.SKF_BF16 and mask is None and is_binary_matrix(arr)
            data = DeviceMatrix(rt.mem.from_host(up), arr.shape, binary=binary)
        if mask is not None and not isinstance(mask, (DeviceMatrix, PackedMask)):
            mask = pack_mask(mask, rt.mem)
        rels.append((i, j, data, mask) + tuple(rel[4:]))
    for t, data in theta_list:
        if isinstance(data, KnownEntries):               # a constraint as its entries: one upload, master dtype
            data = upload_known_entries(data, code, rt.mem)
        if not isinstance(data, (DeviceMatrix, DeviceKnownEntries)):
            arr = np.ascontiguousarray(data, dtype=npd)
            data = DeviceMatrix(rt.mem.from_host(arr), arr.shape)
            data.nnz = int(np.count_nonzero(arr))          # (as DevicePlan counts a host array: the same path either way)
        thetas.append((t, data))
    return rels, thetas


def iterate_rows_lockstep(plans, n_iters=1):
    """Drive the row-block plans of ALL ranks from one process (same device), summing the exchange
    ranges by hand where the ranks of a process group would all-reduce: the single-GPU / emulator
    test vehicle of the row-block schedule."""
    views = [p._exchange_views() for p in plans]

    def exchange(*which):
        for p in plans:
            p.synchronize()
        for w in which:
            ts = [v[w] for v in views]
            if ts[0] is None:
                continue
            total = ts[0].clone()
            for t in ts[1:]:
                total += t
            for t in ts:
                t.copy_(total)
        for p in plans:
            p.synchronize()
    for _ in range(int(n_iters)):
        for p in plans:
            p.stage(nat.SKF_STAGE_CONTRACT)
        exchange(0, 1)
        for p in plans:
            p.stage(nat.SKF_STAGE_BACKBONE)
        exchange(2)
        for p in plans:
            p.stage(nat.SKF_STAGE_ACCUMULATE)
        exchange(3)
        for p in plans:
            p.stage(nat.SKF_STAGE_UPDATE)


def flatten_relations(R, M=None):
    """dict {(i,j): [matrix, ...]} -> [(i, j, matrix, mask)] in dict order, list order
    (the order the reference walks `R`, _dfmf.py:249-251).  A relation given as KnownEntries carries its own pattern of
    known entries: its mask is None whatever M holds."""
    out = []
    for (i, j), mats in R.items():
        for l, m in enumerate(mats):
            mask = None
            if M is not None and M.get((i, j)) is not None and not isinstance(m, KnownEntries):
                mask = M[i, j][l]
            out.append((i, j, m, mask))
    return out


def flatten_thetas(Theta):
    out = []
    for (i, i2), mats in Theta.items():
        for m in mats:
            out.append((i, m))
    return out


def count_objects(obj_types, R):
    """Objects per type from the relation shapes (reference count_objects, _dfmf.py:95-124).
    A mismatch is a hard error here (the reference only logs it and carries on)."""
    from .fusion.base import DataFusionError
    n = {}
    for (i, j), mats in R.items():
        for m in mats:
            for ax, t in enumerate((i, j)):
                have = n.setdefault(t, m.shape[ax])
                if have != m.shape[ax]:
                    raise DataFusionError('Relation matrix R_(%s,%s) dimension mismatch' % (i, j))
    if set(obj_types) != set(n):
        raise DataFusionError('Object type specification mismatch')
    return n
