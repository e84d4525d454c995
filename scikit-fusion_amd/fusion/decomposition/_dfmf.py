"""Functional solver seam of DFMF and of the fold-in transform -- same signatures as the
reference's ``dfmf()`` (_dfmf.py:127-129) and ``transform()`` (_dfmf.py:330-333) -- driving the
device engine.  ``R`` / ``Theta`` are dictionaries keyed by (row_type, col_type) whose values
are LISTS of matrices; the result is ``(G, S)`` with ``G[(t, t)]`` and ``S[(i, j)] = [..]``.

Extra keyword-only engine options (defaults keep the reference behaviour):
  dtype   'f64' (default, parity with the float64 reference) | 'f32'
  G0      dict {(t,t): ndarray} overriding the initialiser (warm start / parity tests), or a `_init.DeviceInit`: the
          draws of a column-mean initialiser, which the bound plan turns into its factors on the device (whole fits only)
"""
import collections
import logging

import numpy as np

from ... import _native as nat
from ..._distributed import world, partition_relations, gather_backbones, sum_over_ranks
from ..._engine import DevicePlan, flatten_relations, flatten_thetas, count_objects
from ._init import initialize, host_view, DeviceInit

log = logging.getLogger('skfusion_amd')


def _as_rs(random_state):
    if isinstance(random_state, np.random.RandomState):
        return random_state
    return np.random.RandomState(random_state)


def _unpack(values, obj_types, rel_list):
    G = {(t, t): values[k] for k, t in enumerate(obj_types)}
    S = {}
    for k, rel in enumerate(rel_list):
        S.setdefault((rel[0], rel[1]), []).append(values[len(obj_types) + k])
    return G, S


def _collect(plan, obj_types, rel_list):
    """(G, S) of the plan: all copies issued, ONE synchronisation, then the read-back."""
    fetched = plan.fetch_results(obj_types, len(rel_list))
    plan.synchronize()
    return _unpack(plan.read_results(fetched), obj_types, rel_list)


def _rel_index(rel_list, target):
    """target = (row, col) or ((row, col), l) -> flat relation index."""
    if isinstance(target[0], tuple):
        pair, l = target
    else:
        pair, l = target, 0
    hits = [k for k, (i, j, _, _) in enumerate(rel_list) if (i, j) == tuple(pair)]
    return hits[l]


class Validation(object):
    """Held-out pairs scored inside one fit (csrc/skf_heldout.h; `DevicePlan.set_heldout`): what the fit is given, and what
    it leaves behind.
    lists: [(target, rows, cols, values)], target = (row_type, col_type) or ((row_type, col_type), l) as for `stopping`;
    the held-out pairs of that relation with their true values, at most one list per relation.  After every iteration the
    device adds up (v - x)^2 over every list and judges the POOLED sum over all lists: an improvement is
    total < best - min_delta (the first total always is); `patience` > 0: that many iterations in a row without one end
    the fit.  The loop stays on the device: `check_every` iterations are issued at a time and only the monitor's state
    words are read in between, so a fit that stops at iteration t runs on to the next multiple of `check_every` -- the
    judge froze at t, and history, best iterate and returned model do not depend on `check_every`.
    restore_best: the fit returns the (G, S) of the best iterate (a device copy taken when it was judged); False: the last.
    Left behind: sqerr (iterations x lists, up to the stop), best_iter (1-based; 0: every total was NaN), n_iter (iterations
    run), stopped."""

    def __init__(self, lists, patience=None, min_delta=0.0, check_every=8, restore_best=True):
        if int(check_every) < 1:
            raise ValueError('check_every must be at least 1')
        if patience is not None and int(patience) < 1:
            raise ValueError('patience must be at least 1 (None: never stop early)')
        if not (float(min_delta) >= 0.0):
            raise ValueError('min_delta must be >= 0')
        self.lists, self.patience, self.min_delta = list(lists), patience, float(min_delta)
        self.check_every, self.restore_best = int(check_every), bool(restore_best)
        self.sqerr = self.best_iter = self.n_iter = self.stopped = None


def _monitored_loop(plan, sharding, validation, max_iter, host_loop):
    """The loop of a fit with held-out lists: chunks of `check_every` iterations, the monitor's words read in between --
    or, where the host is needed every iteration anyway (`host_loop`: callback, stopping, error logging), that loop with a
    chunk of one and the monitor's verdict as one more reason to stop.  Returns the iterations run."""
    done = [0]

    def stopped():
        return plan.monitor(history=False)['stopped']
    if host_loop is not None:
        def step():
            sharding.step(plan, 1)
            done[0] += 1
        host_loop(step, stopped)
        return done[0]
    while done[0] < max_iter:
        n = min(validation.check_every, max_iter - done[0])
        sharding.step(plan, n)
        done[0] += n
        if stopped():
            break
    return done[0]


def _host_loop(step, sqerrs, rel_list, max_iter, stopping, stopping_system, compute_err, on_iter, stop=None):
    """The body of the reference loops with their early-stopping / error logging (_dfmf.py:212-221, 301-322;
    _dfmc.py:270-279, 370-392; fold-in _dfmf.py:367-376, 433-450), one device iteration per pass.
    step(): one iteration; sqerrs(indices): squared reconstruction errors of those relations (summed over the
    ranks of a sharded fit, so that every rank takes the same decision); on_iter(it): the callback hook; stop(): one more
    reason to end the loop, asked before every iteration after the first (a fit with held-out lists: the monitor's verdict)."""
    if stopping_system:
        compute_err = True
    err_t = (None, None)
    err_s = (None, None)
    objective = []
    for it in range(max_iter):
        if it > 1 and stopping and err_t[1] - err_t[0] < stopping[1]:
            log.info("Early stopping: target matrix change < %5.4f", stopping[1])
            break
        if it > 1 and stopping_system and err_s[1] - err_s[0] < stopping_system:
            log.info("Early stopping: matrix system change < %5.4f", stopping_system)
            break
        if it > 0 and stop is not None and stop():
            log.info("Early stopping: held-out error without improvement")
            break
        step()
        if compute_err:
            sq = sqerrs(list(range(len(rel_list))))
            s = 0.
            for (i, j, _, _), v in zip(rel_list, sq):
                e = np.sqrt(v)
                log.info("Relation R_%s,%s norm difference: %5.4f", i, j, e)
                s += e
            log.info("Error (objective function value): %5.4f", s)
            objective.append(s)
            err_s = (s, err_s[0])
            if stopping:
                err_t = (np.sqrt(sq[_rel_index(rel_list, stopping[0])]), err_t[0])
        elif stopping:
            k = _rel_index(rel_list, stopping[0])
            err_t = (np.sqrt(sqerrs([k])[0]), err_t[0])
        if on_iter:
            on_iter(it)
    if compute_err:
        log.info("Violations of optimization objective: %d/%d",
                 int(np.sum(np.diff(objective) > 0)), len(objective))
    return objective


def row_block_plan(variant, rel_list, theta_list, obj_types, n_obj, obj_type2rank, dtype, engine, rank, size):
    """The plan of rank `rank` of `size` in a row-block-sharded fit: all relations listed, each with
    this rank's row block of `_distributed.partition_rows` (or marked absent)."""
    from ..._distributed import partition_rows
    # block boundaries: multiples of the contraction tile for big graphs; bf16 needs multiples of 64
    align = 256 if min(n_obj.values()) >= 4096 else (64 if dtype == 'bf16' else 1)
    blocks, theta_owner = partition_rows(rel_list, theta_list, n_obj, obj_type2rank, align=align, size=size)
    from ..._engine import is_binary_matrix
    local = []
    for (i, j, m, mask), blk in zip(rel_list, blocks):
        mine = [b for b in blk if b[0] == rank]
        info = {'masked': mask is not None, 'col_side': bool(mine) and mine[0][1] == 0}
        if dtype == 'bf16' and mask is None:         # decided on the whole relation: the same path on every rank
            info['binary'] = is_binary_matrix(m)
        if not mine:
            info.update(absent=True, row_begin=0, n_rows=0, col_side=False)
            local.append((i, j, None, None, info))
            continue
        _, a, cnt = mine[0]
        info.update(absent=False, row_begin=a, n_rows=cnt)
        local.append((i, j, np.asarray(m)[a:a + cnt], None if mask is None else np.asarray(mask)[a:a + cnt], info))
    return DevicePlan(obj_types, n_obj, obj_type2rank, local,
                      [t for t, o in zip(theta_list, theta_owner) if o == rank], variant,
                      dtype=dtype, engine=engine, part=(rank, size))


def owned_plan(variant, rel_list, theta_list, obj_types, n_obj, obj_type2rank, dtype, engine, rank, size):
    """The plan of rank `rank` of `size` in a fit sharded by OWNERSHIP (SKF_OPT_OWNED_ROWS): the rank owns the same share
    of the rows of every object type (`_engine.owned_rows`) and holds exactly those rows of every relation whose row type
    it is -- work is 1 / size of every relation, the row-side terms never leave the rank -- and every dense constraint.
    A constraint given as its entries (`_engine.KnownEntries(unstored='zero')`) is sliced the same way: the rank hands over
    the CSR of the owned rows of the constrained type over all columns (an empty (0, n) slice where it owns none), the rows
    its constraint pass multiplies -- never the whole constraint, never a dense form.
    A relation given as its entries (`_engine.KnownEntries`, either kind) is sliced by rows -- `indptr`, `indices` and
    `values` of the owned rows, no dense step -- and only that slice is uploaded; a rank without rows of its row type marks
    it absent.  Every process still holds the WHOLE scipy.sparse matrix / KnownEntries on the host: the initialisers read
    all of it (`_init._KnownView`), only the device sees a slice."""
    from ..._engine import is_binary_matrix, owned_rows, known_lists_pay, KnownEntries, DeviceKnownEntries
    from ..._distributed import same_on_all_ranks
    local = []
    for (i, j, m, mask) in rel_list:
        begin, count, _ = owned_rows(dtype, n_obj[i], rank, size)
        info = {'masked': mask is not None, 'col_side': True, 'row_begin': begin if count else 0, 'n_rows': count,
                'absent': count == 0}
        if isinstance(m, DeviceKnownEntries):
            raise ValueError("relation (%s,%s): an ownership-sharded fit slices the entries on the host (KnownEntries)" % (i, j))
        if isinstance(m, KnownEntries):              # the CSR of the owned rows over all columns, never expanded
            if mask is not None:
                raise ValueError('relation (%s,%s): known entries take no mask' % (i, j))
            info['entries'] = m.unstored
            local.append((i, j, m.row_slice(begin, count) if count else None, None, info))
            continue
        if mask is not None and variant == nat.SKF_DFMC:      # lists of the known entries: one decision for all ranks
            mk = np.asarray(mask, dtype=bool)
            info['known_lists'] = same_on_all_ranks(known_lists_pay(
                mk.size - int(np.count_nonzero(mk)), mk.shape[0], mk.shape[1], int(obj_type2rank[i]), dtype))
        if dtype == 'bf16' and mask is None:         # decided on the whole relation: the same path on every rank
            info['binary'] = is_binary_matrix(m)
        if count == 0:
            local.append((i, j, None, None, info))
            continue
        local.append((i, j, np.asarray(m)[begin:begin + count],
                      None if mask is None else np.asarray(mask)[begin:begin + count], info))
    thetas = []
    for (t, th) in theta_list:
        if isinstance(th, DeviceKnownEntries):
            raise ValueError("constraint on %s: an ownership-sharded fit slices the entries on the host (KnownEntries)" % (t,))
        if isinstance(th, KnownEntries):
            if th.unstored != 'zero' or th.by_col:
                raise ValueError("constraint on %s: entries need unstored='zero', compressed along the rows" % (t,))
            begin, count, _ = owned_rows(dtype, n_obj[t], rank, size)
            th = th.row_slice(begin if count else 0, count)
        thetas.append((t, th))
    return DevicePlan(obj_types, n_obj, obj_type2rank, local, thetas, variant, dtype=dtype, engine=engine,
                      part=(rank, size), owned=True)


# What tells one way of sharing a fit out from another -- everything else is `_fit`, once.  All six take the plan first:
#   make_plan(variant, rel_list, theta_list, obj_types, n_obj, obj_type2rank, dtype, engine) -> the plan of this process
#   attach(plan)                   its communicator, if any
#   load(plan, obj_types, G0)      the initial factors
#   step(plan, n)                  n iterations
#   sqerrs(plan, indices)          squared reconstruction errors of those relations of `rel_list`, the same on every rank
#   collect(plan, obj_types, rel_list) -> (G, S)
_Sharding = collections.namedtuple('_Sharding', 'make_plan attach load step sqerrs collect')


def _fit(sharding, variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type, random_state, dtype, G0, engine,
         stopping, stopping_system, compute_err, callback, validation=None):
    """One fit, shared out as `sharding` says: the body of the reference loops (_dfmf.py:212-322, _dfmc.py:270-392) with the
    arithmetic on the device.  A size mismatch between the relations is reported before anything is drawn from
    `random_state`; the plain loop stays on the device, `_host_loop` runs where the host is needed every iteration."""
    obj_types = list(obj_types)
    n_obj = count_objects(obj_types, R)
    if G0 is None:
        R_first = {k: host_view(v[0]) for k, v in R.items()}
        G0 = initialize(obj_types, n_obj, obj_type2rank, R_first, init_type, _as_rs(random_state))
    rel_list = flatten_relations(R, M)
    plan = sharding.make_plan(variant, rel_list, flatten_thetas(Theta), obj_types, n_obj, obj_type2rank, dtype, engine)
    try:
        sharding.attach(plan)
        sharding.load(plan, obj_types, G0)
        on_iter = (lambda it: callback(*(sharding.collect(plan, obj_types, rel_list) + (it,)))) if callback else None
        host_loop = None
        if callback or stopping or stopping_system or compute_err:
            host_loop = lambda step, stop=None: _host_loop(step, lambda idx: sharding.sqerrs(plan, idx), rel_list, max_iter,
                                                           stopping, stopping_system, compute_err, on_iter, stop)
        if validation is not None:
            return _fit_validated(plan, sharding, validation, obj_types, rel_list, max_iter, host_loop)
        if host_loop is None:
            sharding.step(plan, max_iter)       # whole loop device-resident, no host sync
        else:
            host_loop(lambda: sharding.step(plan, 1))
        return sharding.collect(plan, obj_types, rel_list)
    finally:
        plan.close()


def _fit_validated(plan, sharding, validation, obj_types, rel_list, max_iter, host_loop):
    """The loop and the read-back of a fit with held-out lists (`Validation`), on a loaded whole plan."""
    lists = [(_rel_index(rel_list, target), rows, cols, vals) for target, rows, cols, vals in validation.lists]
    plan.set_heldout(lists, validation.patience or 0, validation.min_delta, capacity=max_iter)
    validation.n_iter = _monitored_loop(plan, sharding, validation, max_iter, host_loop)
    m = plan.monitor()
    validation.stopped = m['stopped']
    validation.best_iter = m['best_iter']
    validation.sqerr = m['history'][:m['stop_iter']] if m['stopped'] else m['history']
    if not (validation.restore_best and m['best_iter'] > 0):
        return sharding.collect(plan, obj_types, rel_list)
    values = [plan.best_factor(t) for t in obj_types] + [plan.best_backbone(k) for k in range(len(rel_list))]
    return _unpack(values, obj_types, rel_list)


def _whole_plan(variant, rel_list, theta_list, obj_types, n_obj, obj_type2rank, dtype, engine):
    return DevicePlan(obj_types, n_obj, obj_type2rank, rel_list, theta_list, variant, dtype=dtype, engine=engine)


def _held_relations_plan(variant, rel_list, theta_list, obj_types, n_obj, obj_type2rank, dtype, engine):
    """The plan of this rank in a relation-sharded fit: the relations and constraints `partition_relations` gives it.
    `plan.held`: the index in `rel_list` of every relation the plan holds, in the plan's order."""
    rank, _ = world()
    rel_owner, theta_owner = partition_relations(rel_list, theta_list, n_obj, obj_type2rank)
    held = [k for k, o in enumerate(rel_owner) if o == rank]
    plan = _whole_plan(variant, [rel_list[k] for k in held], [t for t, o in zip(theta_list, theta_owner) if o == rank],
                       obj_types, n_obj, obj_type2rank, dtype, engine)
    plan.held = held
    return plan


def _load_at_once(plan, obj_types, G0):
    """Every factor with one synchronisation -- or, for the draws of a column-mean initialiser, by the bound plan itself."""
    if isinstance(G0, DeviceInit):
        G0.apply(plan, obj_types)
    else:
        plan.set_factors({t: G0[t, t] for t in obj_types})


def _load_by_type(plan, obj_types, G0):
    for t in obj_types:
        plan.set_factor(t, G0[t, t])


def _attach_or_single(plan):
    if not plan.attach_comm():
        # a single process: every row is owned here and nothing is exchanged -- a genuine communicator of one rank (the
        # null communicator of bench.py --emulate-rank never updates the factors: not for fits)
        plan.attach_single_comm()


def _sqerrs_here(plan, idx):
    return [plan.relation_sqerr(k) for k in idx]


def _sqerrs_of_rows(plan, idx):
    """Every rank holds the squared error of ITS rows (row blocks, owned rows); factors and backbones are replicated."""
    return sum_over_ranks([plan.relation_sqerr(k) for k in idx])


def _sqerrs_of_held(plan, idx):
    """The owner of a relation contributes its error: global relation index -> index in this rank's plan."""
    where = {k: q for q, k in enumerate(plan.held)}
    return sum_over_ranks([plan.relation_sqerr(where[k]) if k in where else 0.0 for k in idx])


def _collect_held(plan, obj_types, rel_list):
    """(G, S) of a relation-sharded fit: the replicated factors, the backbones gathered from their owners (collective)."""
    G = {(t, t): plan.get_factor(t) for t in obj_types}
    backbones = gather_backbones({k: plan.get_backbone(q) for q, k in enumerate(plan.held)}, len(rel_list))
    S = {}
    for k, (i, j, _, _) in enumerate(rel_list):
        S.setdefault((i, j), []).append(backbones[k])
    return G, S


def _attach_group(plan):
    plan.attach_comm()                 # the library issues the exchanges itself (skf_iterate_dist)


_WHOLE = _Sharding(make_plan=_whole_plan, attach=lambda plan: None, load=_load_at_once,
                   step=lambda plan, n: plan.iterate(n), sqerrs=_sqerrs_here, collect=_collect)
_RELATIONS = _Sharding(make_plan=_held_relations_plan, attach=_attach_group, load=_load_by_type,
                       step=lambda plan, n: plan.iterate_sharded(n), sqerrs=_sqerrs_of_held, collect=_collect_held)
_ROWS = _Sharding(make_plan=lambda *graph: row_block_plan(*(graph + world())), attach=_attach_group, load=_load_by_type,
                  step=lambda plan, n: plan.iterate_rows(n), sqerrs=_sqerrs_of_rows, collect=_collect)
_OWNED = _Sharding(make_plan=lambda *graph: owned_plan(*(graph + world())), attach=_attach_or_single, load=_load_by_type,
                   step=lambda plan, n: plan.iterate_dist(n), sqerrs=_sqerrs_of_rows, collect=_collect)


def run_fit_owned(variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type,
                  random_state, dtype, G0, engine, stopping=None, stopping_system=None, compute_err=False,
                  callback=None):
    """One fit sharded by ownership over the ranks of the process group (`shard='owned'`; SURVEY.md 8e, second row, in
    the form with the least exchange): per iteration a rank sends the partial Q of every relation (reduce-scatter), its
    updated factor rows (all-gather) and c x c partial sums -- no E / D exchange (DevicePlan.iterate_dist, the library
    issues the collectives).  Every rank ends with the full (G, S)."""
    return _fit(_OWNED, variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type, random_state, dtype, G0, engine,
                stopping, stopping_system, compute_err, callback)


def run_fit_rows(variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type,
                 random_state, dtype, G0, engine, stopping=None, stopping_system=None, compute_err=False,
                 callback=None):
    """One fit whose relations are cut into balanced ROW BLOCKS over the ranks of the process group
    (SURVEY.md 8e): every rank lists all relations with its own row block (or none), factors are
    replicated, and an iteration is four stages with all-reduces of W / Q, E / D in between
    (`DevicePlan.iterate_rows`).  Every rank ends with the full (G, S)."""
    return _fit(_ROWS, variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type, random_state, dtype, G0, engine,
                stopping, stopping_system, compute_err, callback)


def run_fit_sharded(variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type,
                    random_state, dtype, G0, engine, stopping=None, stopping_system=None, compute_err=False,
                    callback=None):
    """One fit whose relations are partitioned over the ranks of the process group (one GPU
    each): replicated factors, local contractions, ONE all-reduce of the E / D accumulators per
    iteration (second row).  Every rank returns the full (G, S).
    `callback`, `stopping`, `stopping_system` and `compute_err` must be given identically on EVERY rank (as with any
    SPMD launch of the same script): the callback path gathers the backbones collectively, and a callback on one rank
    only would leave the others out of that collective.  The current device of each rank must be set before the
    fit (torch.cuda.set_device(LOCAL_RANK)) for the RCCL reductions."""
    return _fit(_RELATIONS, variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type, random_state, dtype, G0,
                engine, stopping, stopping_system, compute_err, callback)


def run_fits_concurrent(variant, R, M, Theta, obj_types, obj_type2rank, max_iter, dtype, G0_list, engine,
                        n_streams, batch_only=False):
    """The restarts of ONE graph on one GPU, `n_streams` of them at a time -- the reference's `n_jobs` over `n_run`
    (joblib workers, dfmf.py:87-95) for graphs too small to fill the chip.  Where the plans run the schedule for small
    graphs the restarts of a batch share every launch (skf_iterate_batch: the restart is a grid dimension); otherwise each
    runs on a HIP stream of its own: a single fit is then a chain of dependent few-microsecond launches, and several
    chains interleave on the device.  batch_only: None (nothing run) unless the plans take the small-graph schedule -- the
    caller asked for no concurrency (n_jobs = 1) and gets the shared launches only where they are free.  The graph is uploaded once and shared; one host thread per
    stream issues the launches.  Returns
    [(G, S)] in run order; results are identical to sequential runs (each plan is deterministic)."""
    from ..._engine import upload_graph
    obj_types = list(obj_types)
    n_obj = count_objects(obj_types, R)
    rt = nat.get_runtime()
    rel_list, theta_list = upload_graph(flatten_relations(R, M), flatten_thetas(Theta), dtype, rt)
    own_streams = hasattr(rt.mem, 'new_stream')
    out = []
    for k0 in range(0, len(G0_list), max(int(n_streams), 1)):
        plans = []
        try:
            for G0 in G0_list[k0:k0 + max(int(n_streams), 1)]:
                plan = DevicePlan(obj_types, n_obj, obj_type2rank, rel_list, theta_list, variant, dtype=dtype,
                                  engine=engine, stream=rt.mem.new_stream() if own_streams else None)
                plans.append(plan)
                if batch_only and not plan.batchable():        # (decided on the first plan, before a second workspace exists)
                    return None
                if isinstance(G0, DeviceInit):                 # the plan initialises itself (column means on the device)
                    G0.apply(plan, obj_types)
                else:
                    plan.set_factors({t: G0[t, t] for t in obj_types}, sync=False)
            rt.mem.synchronize()                               # the uploads went out on the plans' own streams
            if len(plans) > 1 and DevicePlan.iterate_batch(plans, max_iter):
                pass      # a small graph: every launch served all the restarts of the batch (skf_iterate_batch), one stream
            elif own_streams and len(plans) > 1:
                # one host thread per stream feeds the launches (ctypes releases the GIL inside skf_iterate;
                # a plan is only ever touched by its own thread); the streams run side by side
                import threading
                errors = []

                def drive(plan):
                    try:
                        if getattr(rt.mem, 'device', None) is not None and hasattr(rt.mem, 'torch'):
                            rt.mem.torch.cuda.set_device(rt.mem.device)      # the current device is per thread
                        plan.iterate(max_iter)
                    except Exception as exc:          # surfaced after the join
                        errors.append(exc)
                threads = [threading.Thread(target=drive, args=(plan,)) for plan in plans]
                for th in threads:
                    th.start()
                for th in threads:
                    th.join()
                if errors:
                    raise errors[0]
            else:
                for plan in plans:
                    plan.iterate(max_iter)
            rt.mem.synchronize()
            fetched = [plan.fetch_results(obj_types, len(rel_list)) for plan in plans]
            rt.mem.synchronize()                               # one synchronisation for the read-back of every plan
            for plan, f in zip(plans, fetched):
                out.append(_unpack(plan.read_results(f), obj_types, rel_list))
        finally:
            for plan in plans:
                plan.close()
    return out


def run_fit(variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type, stopping,
            stopping_system, verbose, compute_err, callback, random_state, dtype, G0, engine, validation=None):
    """Shared driver of dfmf / dfmc: the body of the reference loops (_dfmf.py:212-322,
    _dfmc.py:270-392) with the arithmetic on the device."""
    logging.basicConfig(format="%(asctime)s %(levelname)s: %(message)s", level=50 - verbose)
    return _fit(_WHOLE, variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type, random_state, dtype, G0, engine,
                stopping, stopping_system, compute_err, callback, validation)


_SHARDED_FITS = {'relations': run_fit_sharded, 'rows': run_fit_rows, 'owned': run_fit_owned}


def _fit_by_shard(variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type, stopping, stopping_system, verbose,
                  compute_err, callback, random_state, dtype, G0, engine, shard, sparse_constraints, validation=None):
    """The shard dispatch of `dfmf` and `_dfmc.dfmc`: one whole fit on this process (shard None / 'runs'), or this
    process's part of a fit shared out over the process group -- 'relations', 'rows', 'owned' -- which takes dense
    constraints (`refuse_constraint_entries`)."""
    if shard not in _SHARDED_FITS:
        return run_fit(variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type, stopping, stopping_system,
                       verbose, compute_err, callback, random_state, dtype, G0, engine, validation)
    if validation is not None:
        raise ValueError("held-out validation lists need a whole fit on this process (shard='runs'), not shard=%r" % (shard,))
    refuse_constraint_entries(Theta, shard, sparse_constraints)
    logging.basicConfig(format="%(asctime)s %(levelname)s: %(message)s", level=50 - verbose)
    return _SHARDED_FITS[shard](variant, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type, random_state, dtype,
                                G0, engine, stopping, stopping_system, compute_err, callback)


def refuse_constraint_entries(Theta, shard, sparse_constraints=False):
    """The sharded fits take dense constraints: one given as its entries (_engine.KnownEntries) is the caller's mistake --
    the class layer expands it before it gets here.  `sparse_constraints`: the caller says it means them; shard='owned' then
    takes them (every rank hands over the slice of its owned rows, `owned_plan`), the other shards still refuse."""
    from ..._engine import KnownEntries, DeviceKnownEntries
    if sparse_constraints and shard == 'owned':
        return
    for key, mats in (Theta or {}).items():
        if any(isinstance(m, (KnownEntries, DeviceKnownEntries)) for m in mats):
            raise ValueError("constraint %r is given as its entries: shard=%r takes dense constraints (shard='runs' or toarray())"
                             % (key, shard))


def dfmf(R, Theta, obj_types, obj_type2rank, max_iter=10, init_type="random_vcol",
         stopping=None, stopping_system=None, verbose=0, compute_err=False, callback=None,
         random_state=None, n_jobs=1, dtype='f64', G0=None, engine=None, shard=None, sparse_constraints=False, validation=None):
    """Data fusion by matrix factorization -- drop-in for reference ``dfmf`` (_dfmf.py:127).
    ``shard='relations'`` (with an initialised torch.distributed group) partitions the relations
    of this ONE fit over the ranks.  A constraint in ``Theta`` may be an ``_engine.KnownEntries(unstored='zero')`` -- its
    entries as canonical CSR, never expanded -- with shard None / 'runs', and with shard='owned' under
    ``sparse_constraints=True`` (every rank hands over the CSR of its owned rows); any other shard: ValueError.
    ``validation``: a `Validation` -- held-out pairs scored on the device after every iteration, early stopping on their
    pooled squared error and the best iterate returned (shard None / 'runs')."""
    return _fit_by_shard(nat.SKF_DFMF, R, None, Theta, obj_types, obj_type2rank, max_iter, init_type, stopping,
                         stopping_system, verbose, compute_err, callback, random_state, dtype, G0, engine, shard,
                         sparse_constraints, validation)


def _transform_graph(R_ij, target_obj_type, G):
    """(types, n_obj, n_t) of a fold-in: the target + every partner type of the new relations (reference _dfmf.py:342-350)."""
    t = target_obj_type
    sizes = [R_ij[i, j][0].shape[0 if t == i else 1] for i, j in R_ij]
    if len(set(sizes)) > 1:
        from ..base import DataFusionError
        raise DataFusionError("Target object type: %s size mismatch" % t)
    types = [t]
    for (i, j) in R_ij:
        for o in (i, j):
            if o not in types:
                types.append(o)
    n_obj = {t: sizes[0]}
    for o in types[1:]:
        n_obj[o] = G[o, o].shape[0]
    return types, n_obj, sizes[0]


def _freeze_model(plan, types, rel_list, g0, G, S, at_once):
    """Freeze the model (G, S) of one restart into a fold-in plan: `g0` for the target `types[0]`, the fitted factors of
    the partner types, and the l-th backbone of every pair for its l-th new relation.  `at_once`: the factors in one
    `set_factors` without a synchronisation of its own (several plans set up together) instead of one `set_factor` each."""
    factors = [(types[0], g0)] + [(o, G[o, o]) for o in types[1:]]
    if at_once:
        plan.set_factors(dict(factors), sync=False)
    else:
        for o, g in factors:
            plan.set_factor(o, g)
    seen = {}
    for k, (i, j, _, _) in enumerate(rel_list):
        l = seen.get((i, j), 0)
        seen[i, j] = l + 1
        plan.set_backbone(k, S[i, j][l])


def transform_runs(R_ij, Theta_i, target_obj_type, obj_type2rank, models, max_iter=10, init_type="random_c",
                   random_state=None, dtype='f64', G0=None, engine=None):
    """The fold-ins of ONE set of new relations into the models of several restarts -- `models` = [(G, S)] per restart, as
    `transform` takes them -- in shared launches: the reference runs `transform` once per restart on joblib workers
    (dfmf.py:191-199).  The new relations and constraints go to the device ONCE, every restart gets a plan with its frozen
    factors / backbones, and one launch per iteration serves all of them (skf_iterate_batch; plans that do not batch --
    a constraint on the target type -- are iterated one after the other, still on the shared uploads).  G0 of restart k is
    drawn k-th from `random_state` (the order in which the per-restart calls would draw).  Returns [G_target] per restart."""
    from ..._engine import upload_graph
    t = target_obj_type
    types, n_obj, n_t = _transform_graph(R_ij, t, models[0][0])
    rs = _as_rs(random_state)
    if G0 is None:
        R_first = {k: host_view(v[0]) for k, v in R_ij.items()}        # (stored entries are read as such, never expanded)
        G0 = [initialize([t], {t: n_t}, obj_type2rank, R_first, init_type, rs)[t, t] for _ in models]
    rt = nat.get_runtime()
    rel_list, theta_list = upload_graph(flatten_relations(R_ij), flatten_thetas(Theta_i), dtype, rt, fold=True)
    plans = []
    try:
        for (G, S), g0 in zip(models, G0):
            plan = DevicePlan(types, n_obj, obj_type2rank, rel_list, theta_list, nat.SKF_TRANSFORM, dtype=dtype, target=t,
                              engine=engine)
            plans.append(plan)
            _freeze_model(plan, types, rel_list, g0, G, S, at_once=True)
        rt.mem.synchronize()
        if not (len(plans) > 1 and plans[0].batchable() and DevicePlan.iterate_batch(plans, max_iter)):
            for plan in plans:
                plan.iterate(max_iter)
        rt.mem.synchronize()
        return [plan.get_factor(t) for plan in plans]
    finally:
        for plan in plans:
            plan.close()


def transform(R_ij, Theta_i, target_obj_type, obj_type2rank, G, S, max_iter=10,
              init_type="random_c", stopping=None, stopping_system=None, verbose=0,
              compute_err=False, callback=None, random_state=None, dtype='f64', G0=None,
              engine=None):
    """Fold new objects of ``target_obj_type`` into a fitted latent space -- drop-in for
    reference ``transform`` (_dfmf.py:330-458): only the target factor moves, ``G`` of the other
    types and ``S`` (1-element lists per pair) stay frozen.  callback(G_i, iter).  A constraint on the target may be an
    ``_engine.KnownEntries(unstored='zero')``: its entries as canonical CSR, never expanded."""
    logging.basicConfig(format="%(asctime)s %(levelname)s: %(message)s", level=50 - verbose)
    t = target_obj_type
    # object types taking part: the target + every partner type of the new relations
    types, n_obj, n_t = _transform_graph(R_ij, t, G)
    if G0 is None:
        R_first = {k: host_view(v[0]) for k, v in R_ij.items()}        # (stored entries are read as such, never expanded)
        G0 = initialize([t], {t: n_t}, obj_type2rank, R_first, init_type,
                        _as_rs(random_state))[t, t]
    rel_list = flatten_relations(R_ij)
    plan = DevicePlan(types, n_obj, obj_type2rank, rel_list, flatten_thetas(Theta_i),
                      nat.SKF_TRANSFORM, dtype=dtype, target=t, engine=engine)
    try:
        _freeze_model(plan, types, rel_list, G0, G, S, at_once=False)
        if not (callback or stopping or stopping_system or compute_err):
            plan.iterate(max_iter)
        else:
            # reference _dfmf.py:367-376, 433-450: the system error of the NEW relations per iteration and
            # `stopping_system` on its change.  (`stopping` reads an undefined name there -- a NameError at the
            # third iteration; here it is the error change of the named relation, as in dfmf().)
            _host_loop(lambda: plan.iterate(1), lambda idx: _sqerrs_here(plan, idx), rel_list,
                       max_iter, stopping, stopping_system, compute_err,
                       (lambda it: callback(plan.get_factor(t), it)) if callback else None)
        return plan.get_factor(t)
    finally:
        plan.close()
