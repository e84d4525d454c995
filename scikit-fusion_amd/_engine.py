"""Host-side driver of one solver run: builds a plan in ``libskfusion_hip.so`` from the
``R / Theta / M`` dictionaries that arrive at the reference's functional seam
(``dfmf(**params)``, reference _dfmf.py:127; ``dfmc``, _dfmc.py:181; ``transform``,
_dfmf.py:330), keeps every matrix resident in HBM for the whole ``max_iter`` loop and copies
``G`` / ``S`` back once at the end (or per iteration when a callback is installed).
"""
import os
import ctypes as C

import numpy as np

from . import _native as nat
# the consuming side of a fitted model has a module of its own; its names stay importable from here
from ._complete import (DeviceMatrix, DeviceReconstructor, _device_gemm, chain_backbone, device_reconstruct,      # noqa: F401
                        AboveLimit, digit_walk, score_of_key, DeviceCompleter)


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
    ``by_col=True`` (``unstored='zero'`` only): the lists are compressed along the COLUMN type -- `indptr` has n_col + 1
    entries and `indices` are rows, the canonical CSC -- which is what a fold-in whose target is the relation's column type
    hands to the library (SKF_REL_FOLD_CSR: lists compressed along the target's side).  `shape` stays the relation's.
    ``row_fill=a, col_fill=b`` (``unstored='zero'``, row lists only): a relation with MISSING values after its fill -- the
    entries not stored hold a_r * b_c, the stored ones their true values (SKF_REL_FILL_RANK1: the filled matrix is
    a b^T + D with D sparse on the stored pattern; the library forms d = v - a_r b_c itself).  One of the two vectors is
    all ones for every fill strategy of ``Relation``.  ``expand`` gives the dense filled matrix."""

    def __init__(self, indptr, indices, values, shape, fill=0.0, unstored='unknown', by_col=False, row_fill=None, col_fill=None):
        if unstored not in ('unknown', 'zero'):
            raise ValueError("unstored must be 'unknown' or 'zero', not %r" % (unstored,))
        if by_col and unstored != 'zero':
            raise ValueError("lists compressed along the column type need unstored='zero'")
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


def upload_known_entries(ke, dtype, mem):
    """KnownEntries -> DeviceKnownEntries: validated on the host first (DataFusionError before any upload); values in the
    element type of the relation data (SKF_BF16: bf16 bits, rounded as dense data is: f64 -> f32 -> bf16).  Entries whose
    unstored neighbours are zero (SKF_REL_SPARSE_CSR) go up in the master type: SKF_BF16 keeps them as f32."""
    ke.validate()
    code = nat.DTYPES[dtype] if isinstance(dtype, str) else dtype
    vals = np.ascontiguousarray(ke.values, dtype=nat.NP_DTYPE[code])
    if code == nat.SKF_BF16 and ke.unstored != 'zero':
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


def _all_reduce_sum(t):
    """Sum a tensor view over the process group (RCCL for GPU tensors; a gloo group -- CPU tests,
    single-GPU smoke runs -- stages GPU tensors through the host)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return
    if t.is_cuda and dist.get_backend() == 'gloo':
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)


def _exchange(mem, tensors, reduce=None):
    """All-reduce(sum) the given workspace views between two stages of a sharded iteration.
    RCCL: issued on the engine's own stream (stream order replaces host synchronisation).  gloo
    (CPU tests, single-GPU smoke runs) or a caller-supplied `reduce`: bracketed by device syncs."""
    import os
    tensors = [t for t in tensors if t is not None]
    if not tensors:
        return
    if reduce is None:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if dist.get_world_size() <= 1 and not os.environ.get('SKF_FORCE_COLLECTIVES'):
            return
        if tensors[0].is_cuda and dist.get_backend() != 'gloo' and hasattr(mem, 'stream_scope'):
            with mem.stream_scope():
                for t in tensors:
                    dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return
        reduce = _all_reduce_sum
    mem.synchronize()
    for t in tensors:
        reduce(t)
    mem.synchronize()


_RCCL = {}          # (rank, world, identity of the default process group) -> communicator handle (None: RCCL not bound on every rank)


def _group_token(dist):
    """What tells one default process group from the next one with the same (rank, world): the name torch gives every group
    it creates, else the identity of the group object."""
    try:
        pg = dist.distributed_c10d._get_default_group()
        return getattr(pg, 'group_name', None) or id(pg)
    except Exception:
        return None


def release_rccl_comms(runtime=None):
    """Destroy the RCCL communicators this process created (atexit; call it before destroy_process_group when the process
    goes on to create another group -- a later group with the same rank / world never reuses a handle of an earlier one
    either way: the cache is keyed on the group)."""
    for key, comm in list(_RCCL.items()):
        _RCCL.pop(key, None)
        if comm:
            try:
                (runtime or nat.get_runtime()).lib.skf_comm_destroy(comm)
            except Exception:
                pass


def comm_info(rt, comm):
    """dict(rank, world, transport: 'single' | 'rccl' | 'callback' | 'null', transport_ranks) of a communicator handle
    (skf_comm_info; transport_ranks of an RCCL communicator is what ncclCommCount reports)."""
    r, w, k, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    rt.call('skf_comm_info', comm, C.byref(r), C.byref(w), C.byref(k), C.byref(n))
    return {'rank': r.value, 'world': w.value, 'transport': nat.COMM_KIND[k.value], 'transport_ranks': n.value}


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


def _shared_rccl_comm(rt, dist):
    """The process's RCCL communicator for the CURRENT default process group (created once per group, reused by every plan
    and restart), or None when it cannot be had on EVERY rank -- all ranks then agree on the callback path instead of some
    blocking in a broadcast the others never reach.  A failure is remembered for that group only.  Collective: every rank
    of the group must call it."""
    import torch
    rank, world = dist.get_rank(), dist.get_world_size()
    key = (rank, world, _group_token(dist))
    if key in _RCCL:
        return _RCCL[key]
    # (communicators made for EARLIER process groups stay alive until release_rccl_comms() / process exit: a DevicePlan created
    #  under such a group may still hold the handle, and a destroyed handle handed to skf_iterate_dist is a use after free --
    #  a process that cycles through many groups keeps one idle communicator per group, which is the cheaper mistake)
    if not getattr(_shared_rccl_comm, '_atexit', False):
        import atexit
        atexit.register(release_rccl_comms)
        _shared_rccl_comm._atexit = True
    import logging
    log = logging.getLogger('skfusion_amd')
    where = 'cuda' if dist.get_backend() != 'gloo' else 'cpu'

    def all_agree(ok):
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=where)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return int(flag.item()) == 1

    # 1. every rank checks LOCALLY that it can resolve RCCL (ncclGetUniqueId needs no peer) and the ranks agree BEFORE anyone
    #    enters ncclCommInitRank: that call is a rendezvous, and a rank that cannot load the library would leave the others
    #    waiting in it until the transport's own timeout
    mine, ident = None, [None]
    try:
        buf = (C.c_char * 128)()
        rt.call('skf_comm_unique_id', buf)
        mine = bytes(buf)
    except nat.SkfNativeError as exc:
        log.warning('RCCL not bound on rank %d (%s): collectives through torch.distributed', rank, exc)
    if not all_agree(mine is not None):
        _RCCL[key] = None
        return None
    if rank == 0:
        ident[0] = mine
    dist.broadcast_object_list(ident, src=0)
    # 2. the rendezvous itself, bounded: a rank still inside ncclCommInitRank after SKF_COMM_TIMEOUT seconds (default 60)
    #    gives up loudly instead of hanging until the NCCL watchdog fires
    import threading
    comm, box = nat._P(), {}

    device = torch.cuda.current_device() if torch.cuda.is_available() else None

    def create():
        try:
            if device is not None:
                torch.cuda.set_device(device)       # the current device is per THREAD: RCCL binds the communicator to it
            raw = (C.c_char * 128).from_buffer_copy(ident[0])
            rt.call('skf_comm_create', raw, rank, world, C.byref(comm))
            box['ok'] = True
        except nat.SkfNativeError as exc:
            box['error'] = exc
    limit = float(os.environ.get('SKF_COMM_TIMEOUT', '60'))
    th = threading.Thread(target=create, name='skf_comm_create', daemon=True)
    th.start()
    th.join(limit)
    if th.is_alive():
        # (the peers that did get through are now in the all_agree all-reduce below and would wait there for this rank: the
        #  caller must treat this error as fatal for the process group -- let it propagate and the launcher tears the job down)
        raise RuntimeError('skf_comm_create: rank %d of %d still waits in ncclCommInitRank after %.0f s -- the ranks disagree '
                           '(a peer failed or never called it); SKF_COMM_TIMEOUT sets the limit' % (rank, world, limit))
    ok = bool(box.get('ok'))
    if not ok:
        log.warning('skf_comm_create failed on rank %d (%s)', rank, box.get('error'))
    if not all_agree(ok):
        if ok:
            rt.lib.skf_comm_destroy(comm)
        _RCCL[key] = None
        return None
    _RCCL[key] = comm
    return comm


def _torch_collective(mem, ws, dist, rank, world):
    """skf_collective_fn over torch.distributed on views of the workspace `ws`: the transport of gloo groups (CPU tests,
    smoke runs: device views are staged through the host) and the fall-back of a group whose backend takes device tensors
    (nccl = RCCL) when the library could not bind RCCL itself on every rank, or `force_callback` -- there the collective
    runs on the device view directly (the nccl backend rejects host tensors)."""
    def collective(user, op, buf, count, dtype, stream):
        try:
            import torch
            if dtype == nat.SKF_BF16:           # bf16 rows travel as bytes (all-gather only; gloo has no 16-bit integer type)
                npd, count = np.uint8, count * 2
            else:
                npd = nat.NP_DTYPE[dtype]
            es = np.dtype(npd).itemsize
            n = count * (1 if op == 0 else world)
            view = mem.as_tensor(ws, int(buf) - ws.ptr, n * es, npd)
            mem.synchronize()
            on_device = view.is_cuda and dist.get_backend() != 'gloo'
            host = view if on_device else (view.cpu() if view.is_cuda else view)
            if op in (0, 1):              # (reduce-scatter: the all-reduce of the whole buffer covers the owned range)
                dist.all_reduce(host, op=dist.ReduceOp.SUM)
            elif on_device:
                dist.all_gather_into_tensor(host, host[rank * count:(rank + 1) * count].clone())
            else:
                parts = [torch.empty(count, dtype=host.dtype) for _ in range(world)]
                dist.all_gather(parts, host[rank * count:(rank + 1) * count].clone())
                host = torch.cat(parts)
            if on_device:
                torch.cuda.synchronize()      # the backend's own stream: the engine's next launch must see the result
            elif view.is_cuda or host is not view:
                view.copy_(host)
            mem.synchronize()
            return 0
        except Exception:                 # never unwind through the C frames
            import traceback
            traceback.print_exc()
            return 1
    return collective


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
        mem, lib = self.rt.mem, self.rt.lib

        tdesc = (nat.TypeDesc * len(self.types))()
        for k in range(len(self.types)):
            tdesc[k].n_obj, tdesc[k].rank = self.n_obj[k], self.rank[k]
        rdesc = (nat.RelationDesc * max(len(relations), 1))()
        csr = []                                         # (relation, DeviceKnownEntries): skf_plan_set_known_entries
        self.local_rows = []                             # rows of every relation this plan holds (its block, or all of them)
        # relations with missing values kept as lists: {relation: the constant beneath its unknown entries (KnownEntries.fill),
        # or None for entries plus rank one} -- what the column-mean initialisers need beside the lists (the `_filled` entry points)
        self.rel_over_fill = {}
        for k, rel in enumerate(relations):
            i, j, data, mask = rel[:4]
            block = rel[4] if len(rel) > 4 else None
            rdesc[k].row_type, rdesc[k].col_type = self.index[i], self.index[j]
            self.local_rows.append(int(block['n_rows']) if block is not None else n_obj[i])
            if block is not None and block.get('absent') and block.get('entries'):
                # row ownership, a relation given as its entries, no row of it here: no lists, only the flags
                if not owned:
                    raise ValueError('relation (%s,%s): known entries take a row block under row ownership only' % (i, j))
                rdesc[k].flags = nat.SKF_REL_ABSENT | (nat.SKF_REL_SPARSE_CSR if block['entries'] == 'zero'
                                                       else nat.SKF_REL_KNOWN_CSR)
                continue
            if isinstance(data, (KnownEntries, DeviceKnownEntries)):
                # the known entries only (SKF_REL_KNOWN_CSR), or the stored entries of a relation that is zero elsewhere
                # (SKF_REL_SPARSE_CSR): no dense form, no mask; always kept as lists.  Row ownership: the CSR of the owned
                # rows, indptr rebased to 0, columns over the whole column type
                if mask is not None or (block is not None and not owned):
                    raise ValueError('relation (%s,%s): known entries take no mask and no row block' % (i, j))
                if tuple(data.shape) != (self.local_rows[k], n_obj[j]):
                    raise ValueError('relation (%s,%s) dimension mismatch: %r vs object counts (%d,%d)'
                                     % (i, j, tuple(data.shape), self.local_rows[k], n_obj[j]))
                if block is not None:
                    rdesc[k].row_begin, rdesc[k].n_rows = int(block['row_begin']), self.local_rows[k]
                dev = data if isinstance(data, DeviceKnownEntries) else upload_known_entries(data, self.dtype, mem)
                self._keep_rel.append(dev)
                if variant == nat.SKF_TRANSFORM and dev.unstored == 'zero':
                    # a fold-in: the stored entries compressed along the target's side (SKF_REL_FOLD_CSR)
                    if dev.row_fill is not None:
                        raise ValueError('relation (%s,%s): a filled relation with missing values is for fits, not fold-ins' % (i, j))
                    if dev.by_col != (j == target and i != target):
                        raise ValueError('relation (%s,%s): a fold-in takes the lists compressed along the target %s'
                                         % (i, j, target))
                    rdesc[k].flags |= nat.SKF_REL_FOLD_CSR
                    rdesc[k].known_bound = dev.known
                    csr.append((k, dev))
                    continue
                if dev.by_col:
                    raise ValueError('relation (%s,%s): lists compressed along the column type are for fold-ins' % (i, j))
                rdesc[k].flags |= nat.SKF_REL_SPARSE_CSR if dev.unstored == 'zero' else nat.SKF_REL_KNOWN_CSR
                if dev.row_fill is not None:            # a filled relation with missing values: entries plus rank one
                    rdesc[k].flags |= nat.SKF_REL_FILL_RANK1
                rdesc[k].known_bound = dev.known
                csr.append((k, dev))
                if dev.unstored != 'zero':
                    self.rel_over_fill[k] = float(dev.fill)
                elif dev.row_fill is not None:
                    self.rel_over_fill[k] = None
                continue
            rows_here = n_obj[i]
            if block is not None:
                rows_here = int(block['n_rows'])
                rdesc[k].row_begin, rdesc[k].n_rows = int(block['row_begin']), rows_here
                rdesc[k].flags = ((nat.SKF_REL_ABSENT if block.get('absent') else 0) |
                                  (0 if block.get('col_side', True) else nat.SKF_REL_NO_COL_SIDE) |
                                  (nat.SKF_REL_MASKED if block.get('masked') else 0))
                if block.get('absent'):
                    if block.get('known_lists'):
                        rdesc[k].flags |= nat.SKF_REL_KNOWN_LISTS
                    continue
            if isinstance(data, DeviceMatrix):
                arr, buf, ld = data, data.buf, data.ld
                if data.binary and mask is None and self.dtype == nat.SKF_BF16:
                    rdesc[k].flags |= nat.SKF_REL_BINARY
            else:
                arr = np.ascontiguousarray(data, dtype=self.np_dtype)
                if arr.ndim != 2:
                    raise ValueError('relation %d is not a matrix' % k)
                # SKF_BF16: a 0 / 1 relation is kept as a bitmap on the device (1/16 of the bytes per iteration).  A row
                # block carries the verdict on the WHOLE relation (`binary`), so that every rank of a row-sharded fit
                # takes the same contraction path for it
                if self.dtype == nat.SKF_BF16 and mask is None:
                    binary = block['binary'] if (block is not None and 'binary' in block) else is_binary_matrix(arr)
                    if binary:
                        rdesc[k].flags |= nat.SKF_REL_BINARY
                # SKF_BF16: relations are handed over as bf16 bit patterns
                up = nat.to_bf16_bits(arr) if self.dtype == nat.SKF_BF16 else arr
                buf, ld = mem.from_host(up), arr.shape[1]
            if tuple(arr.shape) != (rows_here, n_obj[j]):
                raise ValueError('relation (%s,%s) dimension mismatch: %r vs object counts (%d,%d)'
                                 % (i, j, tuple(arr.shape), rows_here, n_obj[j]))
            self._keep_rel.append(buf)
            rdesc[k].data, rdesc[k].ld = buf.ptr, ld
            if isinstance(mask, PackedMask):             # packed bits already in HBM (upload_graph)
                if tuple(mask.shape) != tuple(arr.shape):
                    raise ValueError('mask shape mismatch for relation (%s,%s)' % (i, j))
                self._keep_rel.append(mask.buf)
                rdesc[k].mask, rdesc[k].mask_ld = mask.buf.ptr, mask.ld
                rdesc[k].flags |= nat.SKF_REL_MASK_BITS
                rdesc[k].known_bound = mask.known
            elif isinstance(mask, DeviceMatrix):         # uint8 bytes already in HBM (device-generated data)
                if tuple(mask.shape) != tuple(arr.shape):
                    raise ValueError('mask shape mismatch for relation (%s,%s)' % (i, j))
                self._keep_rel.append(mask.buf)
                rdesc[k].mask, rdesc[k].mask_ld = mask.buf.ptr, mask.ld
                rdesc[k].known_bound = mask.known
            elif mask is not None:
                pm = pack_mask(mask, mem)
                if pm.shape != arr.shape:
                    raise ValueError('mask shape mismatch for relation (%s,%s)' % (i, j))
                self._keep_rel.append(pm.buf)
                rdesc[k].mask, rdesc[k].mask_ld = pm.buf.ptr, pm.ld
                rdesc[k].flags |= nat.SKF_REL_MASK_BITS
                rdesc[k].known_bound = pm.known
            if sparse_known is False or (block is not None and not block.get('known_lists')):
                rdesc[k].known_bound = 0
            if block is not None and block.get('known_lists'):       # (row ownership: decided for all ranks alike by the caller)
                rdesc[k].flags |= nat.SKF_REL_KNOWN_LISTS
        hdesc = (nat.ThetaDesc * max(len(thetas), 1))()
        theta_csr = []                                   # (constraint, DeviceKnownEntries): skf_plan_set_constraint_entries
        self.theta_rows = []                             # rows of every constraint kept here (the owned rows of a slice, or all)
        for k, (t, data) in enumerate(thetas):
            self.theta_rows.append(int(n_obj[t]))
            if isinstance(data, (KnownEntries, DeviceKnownEntries)):
                # the stored entries of a constraint that is zero elsewhere (skf_theta_desc.data == NULL): no dense form,
                # always kept as lists; values in the master type
                if data.unstored != 'zero' or data.by_col:
                    raise ValueError("constraint on %s: entries need unstored='zero', compressed along the rows" % (t,))
                if owned:           # the rows [begin, begin + count) this part owns, over all columns
                    self.theta_rows[k] = owned_rows(self.dtype, n_obj[t], part[0], part[1], self.rt)[1]
                if tuple(data.shape) != (self.theta_rows[k], n_obj[t]):
                    raise ValueError('constraint on %s dimension mismatch: %r vs (%d,%d)'
                                     % (t, tuple(data.shape), self.theta_rows[k], n_obj[t]))
                dev = data if isinstance(data, DeviceKnownEntries) else upload_known_entries(data, self.dtype, mem)
                self._keep.append(dev)
                hdesc[k].type, hdesc[k].data, hdesc[k].ld, hdesc[k].nnz = self.index[t], None, 0, dev.known
                theta_csr.append((k, dev))
                continue
            if isinstance(data, DeviceMatrix):           # master dtype, already in HBM
                if tuple(data.shape) != (n_obj[t], n_obj[t]):
                    raise ValueError('constraint on %s dimension mismatch' % (t,))
                self._keep.append(data.buf)
                hdesc[k].type, hdesc[k].data, hdesc[k].ld = self.index[t], data.buf.ptr, data.ld
                hdesc[k].nnz = _sparse_bound(getattr(data, 'nnz', 0), n_obj[t])
                continue
            arr = np.ascontiguousarray(data, dtype=self.np_dtype)
            if arr.shape != (n_obj[t], n_obj[t]):
                raise ValueError('constraint on %s dimension mismatch' % (t,))
            buf = mem.from_host(arr)
            self._keep.append(buf)
            hdesc[k].type, hdesc[k].data, hdesc[k].ld = self.index[t], buf.ptr, arr.shape[1]
            # a sparse constraint (lambda I, a few must-link pairs per object, dicty's ppi) is kept as CSR on the device
            hdesc[k].nnz = _sparse_bound(int(np.count_nonzero(arr)), n_obj[t])
        opt = nat.Options(self.dtype, variant, self.index[target] if target is not None else -1,
                          nat.SKF_ENGINE_MFMA if engine is None else engine,
                          part[0] if part else 0, part[1] if part else 0,
                          (nat.SKF_OPT_OWNED_ROWS | (nat.SKF_OPT_THETA_OWNED_ROWS if theta_csr else 0)) if owned else 0)
        self.owned = bool(owned)
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

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def upload_graph(rel_list, theta_list, dtype, runtime=None):
    """Relations / masks / constraints to HBM ONCE, as DeviceMatrix entries that any number of plans can
    share (concurrent restarts of one graph): same conversions as DevicePlan applies to host arrays."""
    rt = runtime or nat.get_runtime()
    code = nat.DTYPES[dtype] if isinstance(dtype, str) else dtype
    npd = nat.NP_DTYPE[code]
    rels, thetas = [], []
    for rel in rel_list:
        i, j, data, mask = rel[:4]
        if isinstance(data, KnownEntries):
            rels.append((i, j, upload_known_entries(data, code, rt.mem), mask) + tuple(rel[4:]))
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
