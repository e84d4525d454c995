"""Communicator glue of the sharded fits: the torch.distributed exchanges of the staged iterations, the RCCL rendezvous with
its per-group cache, and the callback transport that runs the library's collectives through torch.distributed.  Nothing
here knows about a plan; `_engine.DevicePlan.attach_comm` is the caller, and `_engine` re-exports every name."""
import os
import ctypes as C

import numpy as np

from . import _native as nat


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
