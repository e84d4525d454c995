"""``Dfmf`` and ``DfmfTransform`` -- the class layer of the drop-in boundary.

Same constructor keywords, ``fuse`` / ``transform`` entry points and result containers as the
reference (``skfusion/fusion/decomposition/dfmf.py``: Dfmf :18-106, DfmfTransform :118-204).
What changes is where the arithmetic runs: each of the ``n_run`` restarts is one device plan
in ``libskfusion_hip.so`` (the reference ships every run to a joblib worker, dfmf.py:87-95).
Engine-specific keywords (``dtype``) are additions with behaviour-preserving defaults.
"""
from collections import defaultdict
from itertools import product
from numbers import Number

import numpy as np

from ..base import FusionFit, FusionTransform
from ..._distributed import my_runs, gather_runs
from ..._engine import count_objects
from . import _dfmf
from ._init import initialize, host_view

__all__ = ['Dfmf', 'DfmfTransform']


def _random_state(obj):
    return obj if isinstance(obj, np.random.RandomState) else np.random.RandomState(obj)


SPARSE_RULE = 4.0       # density * max(rank_row, rank_col) at which the entry lists stop paying
FOLD_MIN_CELLS = 1 << 20       # fold-ins, default rule: below this many cells the dense upload is free and nothing changes
LIST_MAX_RANK, LIST_MAX_ENTRIES = 1024, 2000000000      # the limits of the library's entry lists


def _max_rank(relation):
    return max(int(relation.row_type.rank), int(relation.col_type.rank))


def _cells(relation):
    return float(relation.data.shape[0]) * float(relation.data.shape[1])


def _listable(relation, rank, nnz, constraint=False):
    """What every entry-list form asks of a scipy.sparse relation: no preprocessor, two different object types (a
    constraint: one type with itself), and the limits of the library's lists for `rank` and its `nnz` entries."""
    if relation.preprocessor or (relation.row_type == relation.col_type) != constraint:
        return False
    return rank <= LIST_MAX_RANK and nnz <= LIST_MAX_ENTRIES


def _within_rule(relation, rank, nnz):
    """density * rank <= SPARSE_RULE: where a pass over the entry lists still beats the dense one."""
    cells = _cells(relation)
    return cells > 0 and nnz / cells * rank <= SPARSE_RULE


def _sparse_enough(relation, rank, nnz):
    """The default rule of the fits (`sparse_relations` None): `_within_rule`, for relations beyond the
    limits of the small-graph schedule only (``skf_small_graph_limits``: below them an iteration is bound by its launches,
    the three-launch schedule is the measured path and the lists would take the graph off it)."""
    from ..._engine import small_graph_limits
    lim = small_graph_limits()
    if rank <= lim['max_rank'] and max(relation.data.shape) <= lim['max_objects']:
        return False
    return _within_rule(relation, rank, nnz)


def known_entries_apply(relation, known_entries):
    """Whether `relation` enters the fit as its known entries only (``Relation(..., unstored='unknown')`` on the list path
    of Dfmc: asked for by the caller, no preprocessor, fill 'mean' or a number, row type rank <= 1024 and at most 2e9
    entries -- the limits of the library's known-entry lists).  Otherwise such a relation is expanded to its MaskedArray.
    The answer depends on the whole relation only, so every rank of a shard='owned' fit gives the same one."""
    if not (known_entries and relation.is_known_entries()):
        return False
    if not _listable(relation, int(relation.row_type.rank), relation.data.nnz):
        return False
    return isinstance(relation.fill_value, Number) or relation.fill_value == 'mean'


def stored_entries_apply(relation, sparse_relations, shard='runs'):
    """Whether a ``scipy.sparse`` relation with ``unstored='zero'`` enters the fit as its stored entries (never expanded):
    shard='runs' or 'owned' (there every rank uploads the CSR of its owned rows; the decision reads the whole relation's
    shape, nnz and ranks only, so it is the same on every rank; 'rows' / 'relations' expand), no preprocessor, row type !=
    column type, ranks <= 1024 and at most 2e9 entries (the limits of the
    library's lists), and sparse enough -- `sparse_relations` None: density * max(rank_row, rank_col) <= 4, the rule of the
    known-entry lists, for relations beyond the limits of the small-graph schedule (a rank above 64 or more than 8192
    objects on a side, ``skf_small_graph_limits``: below them an iteration is bound by its launches, the three-launch
    schedule is the measured path and the lists would take the graph off it); True: whenever eligible; False: never
    (``toarray()``, as before the sparse path existed)."""
    if sparse_relations is False or shard not in ('runs', 'owned') or not relation.is_zero_unstored():
        return False
    rank, nnz = _max_rank(relation), int(relation.data.nnz)
    if not _listable(relation, rank, nnz):
        return False
    return bool(sparse_relations) or _sparse_enough(relation, rank, nnz)


def filled_entries_apply(relation, sparse_relations, shard='runs', variant='dfmf'):
    """Whether a ``scipy.sparse`` relation with ``unstored='unknown'`` enters the fit as entries plus rank one
    (``Relation.filled_entries``: the filled matrix is a b^T + D, never expanded): shard='runs', no preprocessor, two
    different object types, every stored value finite (a stored NaN / inf takes part in the fill: the dense path's job),
    at least one entry NOT stored (a MaskedArray that masks nothing follows numpy.ma's other rules, ``_fill_lines``), ranks
    <= 1024 and at most 2e9 entries.  `variant` 'dfmf': every fill value; 'dfmc': 'row_mean' / 'col_mean' only -- they leave
    no mask, so the relation is an unmasked one of the DFMC plan ('mean' and numbers keep their mask and go to
    ``known_entries_apply``).  `sparse_relations` follows the rule of ``stored_entries_apply``: None: density *
    max(rank_row, rank_col) <= 4 beyond the small-graph limits; True: whenever eligible; False: never."""
    if sparse_relations is False or shard != 'runs' or not relation.is_known_entries():
        return False
    if isinstance(relation.fill_value, Number) or relation.fill_value == 'mean':
        if variant != 'dfmf':
            return False
    elif relation.fill_value not in ('row_mean', 'col_mean'):
        return False
    rank, cells = _max_rank(relation), _cells(relation)
    if not _listable(relation, rank, int(relation.data.nnz)) or cells <= 0:
        return False
    import scipy.sparse
    csr = scipy.sparse.csr_matrix(relation.data, copy=True)
    csr.sum_duplicates()                                # (the stored pattern: duplicates are one entry)
    nnz = int(csr.indices.size)
    if nnz >= cells or not np.isfinite(csr.data).all():
        return False
    return bool(sparse_relations) or _sparse_enough(relation, rank, nnz)


def constraint_entries_apply(relation, sparse_constraints, shard='runs'):
    """Whether a ``scipy.sparse`` constraint (row type == column type) with ``unstored='zero'`` goes to the device as its
    entries (never expanded): shard='runs' or 'owned' (there every rank hands over the CSR of its owned rows; the decision
    reads the whole constraint's shape and nnz only, so it is the same on every rank; 'rows' / 'relations' expand), no
    preprocessor, finite stored values and at most 2e9 of them.
    `sparse_constraints` True: whenever eligible; False: never (``toarray()``); None: when nnz <= n * n / the library's own
    divisor (``small_graph_limits()``: up to there the dense-fed form is compacted to the same lists, so nothing changes but
    the hand-over) -- a denser one is expanded and takes the dense product, the measured path at that density."""
    if sparse_constraints is False or shard not in ('runs', 'owned') or not relation.is_zero_unstored():
        return False
    nnz = int(relation.data.nnz)
    if not _listable(relation, 0, nnz, constraint=True):        # (no lists by rank here: a constraint multiplies a factor)
        return False
    if not np.isfinite(relation.data.data).all():               # (a stored NaN / inf is filled: the dense path's job)
        return False
    if sparse_constraints:
        return True
    from ..._engine import small_graph_limits
    n = int(relation.data.shape[0])
    return nnz <= n * n // small_graph_limits()['constraint_nnz_divisor']


def fold_entries_apply(relation, sparse_relations):
    """Whether a ``scipy.sparse`` relation with ``unstored='zero'`` enters a fold-in (``DfmfTransform``) as its stored
    entries, compressed along the target's side and never expanded: no preprocessor, two different object types, ranks
    <= 1024 and at most 2e9 entries (the limits of the library's lists).  `sparse_relations` True: whenever eligible;
    False: never; None: when also density * max(rank_row, rank_col) <= SPARSE_RULE (the fit's constant: a dense-fed
    preparation streams every cell once, a list-fed one gathers a c-wide row per entry, the trade of the fit's passes;
    DESIGN.md section 2 says what was measured for the fold-in) and the relation has at least 2^20 cells."""
    if sparse_relations is False or not relation.is_zero_unstored():
        return False
    rank, nnz = _max_rank(relation), int(relation.data.nnz)
    if not _listable(relation, rank, nnz):
        return False
    if sparse_relations:
        return True
    return _cells(relation) >= FOLD_MIN_CELLS and _within_rule(relation, rank, nnz)


def graph_matrices(fusion_graph, with_masks=False, device_dtype=None, known_entries=False, sparse_relations=False,
                   shard='runs', sparse_constraints=False, variant='dfmf'):
    """FusionGraph -> (R, Theta[, M]) dictionaries in the reference's walking order
    (dfmf.py:70-85, dfmc.py:70-93): pairs from product(object_types, repeat=2), each relation
    filled, then preprocessed; relations between two different types go to R, same-type
    relations are constraints (Theta).  For a masked result the raw ``.data`` is used and,
    with ``with_masks``, the mask is kept as the completion mask.
    ``device_dtype``: relations (not constraints) without a preprocessor are filled ON THE DEVICE and enter the
    dictionaries as device-resident matrices of that engine dtype (``Relation.filled_device``).
    ``known_entries`` (Dfmc, shard='runs' / 'owned'): relations given as their known entries enter as ``_engine.KnownEntries`` with
    mask None where ``known_entries_apply`` says so (never filled on the device: nothing unknown is stored).
    ``sparse_relations`` / ``shard``: scipy.sparse relations whose unstored entries are zero enter as their stored entries
    (``_engine.KnownEntries`` with ``unstored='zero'``, mask None) where ``stored_entries_apply`` says so, and
    ``sparse_constraints``: scipy.sparse constraints as their entries where ``constraint_entries_apply`` says so.
    scipy.sparse relations whose unstored entries are UNKNOWN enter as entries plus rank one (``Relation.filled_entries``,
    mask None) where ``filled_entries_apply`` says so for `variant` ('dfmf' | 'dfmc'), ahead of the dense ``filled()``."""
    R, Theta, M = {}, {}, {}
    for row_type, col_type in product(fusion_graph.object_types, repeat=2):
        for relation in fusion_graph.get_relations(row_type, col_type):
            mask = None
            if known_entries_apply(relation, known_entries):
                data = relation.known_entries()
            elif stored_entries_apply(relation, sparse_relations, shard):
                data = relation.stored_entries()
            elif constraint_entries_apply(relation, sparse_constraints, shard):
                data = relation.constraint_entries()
            elif filled_entries_apply(relation, sparse_relations, shard, variant):
                data = relation.filled_entries()
            elif device_dtype and not relation.preprocessor and relation.row_type != relation.col_type:
                data, mask = relation.filled_device(device_dtype)
            else:
                data = relation.filled()
                if relation.preprocessor:
                    data = relation.preprocessor(data)
                if np.ma.is_masked(data):
                    mask = data.mask
                    data = data.data
            key = (relation.row_type, relation.col_type)
            if relation.row_type != relation.col_type:
                R.setdefault(key, []).append(data)
                M.setdefault(key, []).append(mask)
            else:
                Theta.setdefault(key, []).append(data)
    return (R, Theta, M) if with_masks else (R, Theta)


def initial_factors(R, object_types, rank, init_type, random_state, n_run, on_device=False):
    """G0 of every restart, drawn in run order from the ONE shared RandomState (the reference
    passes the same generator object to all runs, dfmf.py:92, consumed sequentially for
    n_jobs=1).  Every rank draws all of them so that the result of run k does not depend on how
    many GPUs share the work.
    `on_device` (a column-mean initialiser, `init_device_wanted` and `init_device_covered`): the draws only -- one
    `_init.DeviceInit` per restart, which the restart's plan turns into its factors after bind; the stream is consumed as
    the host initialiser consumes it, and the relations are never read here."""
    n_obj = count_objects(object_types, R)
    if on_device:
        from ._init import draw_positions, DeviceInit
        shapes = {k: tuple(v[0].shape) for k, v in R.items()}
        pools = {}                               # column rankings of `random_c` from the device norms, shared by the restarts
        return [DeviceInit(draw_positions(object_types, rank, shapes, init_type, random_state), init_type, pools)
                for _ in range(n_run)]
    # ('random' never reads the relations: they may live on the device already, `device_fill`)
    R_first = {} if init_type == 'random' else {k: host_view(v[0]) for k, v in R.items()}
    pools = {}                                   # column rankings of `random_c`, shared by the restarts (R_first stays alive here)
    return [initialize(object_types, n_obj, rank, R_first, init_type, random_state, pools)
            for _ in range(n_run)]


INIT_DEVICE_MIN = 1 << 34   # init_device=None: gathered elements (sum of n_rows * take * c over the oriented views) from which the
                            # device initialiser runs -- about two minutes of the host initialiser at the 1.5e8 elements/s
                            # measured for it (profiles/init_device.txt); every test and bench.py path stays below it


def _first_relations(fusion_graph):
    """The first relation of every pair of different object types (reference _dfmf.py:191: the one the initialisers
    read), in the walking order of `graph_matrices`."""
    for row_type, col_type in product(fusion_graph.object_types, repeat=2):
        if row_type != col_type:
            for relation in fusion_graph.get_relations(row_type, col_type):
                yield relation
                break


INIT_KNOWN_MIN = 1 << 33    # init_device=None, relations with missing values kept as lists: the work of the host initialiser
                            # (`init_known_work`: entries walked + cells of the column buffers) from which the device
                            # initialiser runs -- about two minutes of `_init._KnownView` at the 7.1e7 entries/s measured for
                            # its row means, both orientations averaged (profiles/init_known.txt; the column buffers fill
                            # faster); every test, tool default and bench.py path stays below it


def _kept_as_lists(rel, fuser):
    """Whether a first relation with missing values (``unstored='unknown'``) enters this fit as lists -- its known entries
    (Dfmc) or entries plus rank one --, as `graph_matrices` will decide: the host initialiser then reads it through
    `_init._KnownView`, and gathers nothing."""
    if not rel.is_known_entries():
        return False
    variant = getattr(fuser, '_variant', 'dfmf')
    if variant == 'dfmc' and known_entries_apply(rel, fuser.shard in ('runs', 'owned')):
        return True
    return filled_entries_apply(rel, getattr(fuser, 'sparse_relations', None), fuser.shard, variant)


def init_device_work(fusion_graph, fuser=None):
    """What the host initialiser gathers: sum over the oriented views of n_rows * take * c elements (relations it reads
    as matrices; with `fuser`: not those `init_known_work` counts)."""
    total = 0
    for rel in _first_relations(fusion_graph):
        if fuser is not None and _kept_as_lists(rel, fuser):
            continue
        n_r, n_c = rel.data.shape
        total += n_r * int(.2 * n_c) * int(rel.row_type.rank) + n_c * int(.2 * n_r) * int(rel.col_type.rank)
    return total


def init_known_work(fusion_graph, fuser):
    """What the host initialiser walks for the relations with missing values kept as lists (`_init._KnownView`): per
    oriented view one pass over all stored entries per factor column, c * nnz, and for `random_c` one dense column buffer
    per column of the view, n * m."""
    total = 0
    for rel in _first_relations(fusion_graph):
        if not _kept_as_lists(rel, fuser):
            continue
        n_r, n_c = rel.data.shape
        total += int(rel.data.nnz) * (int(rel.row_type.rank) + int(rel.col_type.rank))
        if fuser.init_type == 'random_c':
            total += 2 * n_r * n_c
    return total


def init_device_wanted(fuser):
    """Whether the fit may initialise on the device, as far as the graph alone tells (before any matrix is formed):
    `init_device` is not False, a column-mean initialiser, whole relations on this process (shard='runs'), no preprocessor
    on a relation between two types (it would have to run on the host first), every first relation of a pair with at least
    5 columns in both orientations (fewer: take = 0 and the reference's mean of nothing, NaN -- the host keeps that), and
    -- `init_device=None` -- at least INIT_DEVICE_MIN gathered elements, or at least INIT_KNOWN_MIN entries walked through
    relations with missing values kept as lists.  `init_device_covered` has the last word."""
    from ._init import COLUMN_MEAN_TYPES
    want = getattr(fuser, 'init_device', None)
    if want is False or fuser.init_type not in COLUMN_MEAN_TYPES or fuser.shard != 'runs':
        return False
    graph = fuser.fusion_graph
    if any(rel.preprocessor for rel in graph.relations if rel.row_type != rel.col_type):
        return False
    if any(min(rel.data.shape) < 5 for rel in _first_relations(graph)):
        return False
    return bool(want) or init_device_work(graph, fuser) >= INIT_DEVICE_MIN or init_known_work(graph, fuser) >= INIT_KNOWN_MIN


def init_device_covered(R, M=None):
    """... and as far as the matrices tell: the first relation of every pair in a form the device initialiser reads --
    unmasked (a relation given as a MaskedArray initialises on the host), and dense (host or device), the stored entries of
    a relation that is zero elsewhere, or a relation with missing values kept as lists compressed by row: its known entries
    (``unstored='unknown'``, Dfmc) or entries plus rank one (`row_fill` set).  Lists compressed by column stay uncovered."""
    from ..._engine import KnownEntries, DeviceKnownEntries
    for key, mats in R.items():
        if M is not None and M.get(key) is not None and M[key][0] is not None:
            return False
        m = mats[0]
        if isinstance(m, (KnownEntries, DeviceKnownEntries)) and m.by_col:
            return False
    return True


def _fills_without_mask(fusion_graph):
    """Every relation between two types is a plain ndarray or a scipy.sparse matrix whose unstored entries are zero: no
    fill leaves a mask behind, so what `init_device_wanted` says holds for the filled matrices too."""
    return all(isinstance(rel.data, np.ndarray) and not np.ma.isMaskedArray(rel.data) or rel.is_zero_unstored()
               for rel in fusion_graph.relations if rel.row_type != rel.col_type)


def device_fill_dtype(fuser):
    """The engine dtype when the fill strategies of the relations may run on the device: asked for
    (`device_fill=True`), whole relations on this process (shard='runs'), and an initialiser that does not read the
    filled values on the host: 'random', or a column-mean initialiser (`random_c` / `random_vcol`) when it will run on the
    device (`init_device_wanted`, and relations whose fill leaves no mask: the decision cannot be taken back once the
    filled matrix exists in HBM only)."""
    if not (getattr(fuser, 'device_fill', False) and fuser.shard == 'runs'):
        return None
    if fuser.init_type == 'random' or (init_device_wanted(fuser) and _fills_without_mask(fuser.fusion_graph)):
        return fuser.dtype
    return None


def concurrent_streams(fuser):
    """`n_jobs` -> how many of the `n_run` restarts share this GPU concurrently, each on a stream of
    its own (0: one after the other).  The reference hands the restarts to `n_jobs` joblib workers
    (dfmf.py:87-95); here they stay in one process.  Only the plain loop qualifies (no callback /
    stopping / error logging, which need the host every iteration), and a process group shares
    the restarts out over the GPUs instead."""
    from ..._distributed import world
    if fuser.n_run < 2 or fuser.callback or fuser.stopping or fuser.stopping_system or fuser.compute_err:
        return 0
    if fuser.shard != 'runs' or world()[1] > 1:
        return 0
    nj = fuser.n_jobs
    if nj is None or nj in (0, 1):
        return 0
    return min(fuser.n_run, 16 if nj < 0 else int(nj), 16)


def shared_launches(fuser):
    """Several restarts, the plain loop, one GPU: candidates for skf_iterate_batch (every launch serves all restarts of a
    small graph; results identical to one restart after the other, so `n_jobs` need not ask for it)."""
    from ..._distributed import world
    if fuser.n_run < 2 or fuser.callback or fuser.stopping or fuser.stopping_system or fuser.compute_err:
        return False
    if not (fuser.shard == 'runs' and world()[1] <= 1 and fuser.dtype in ('f64', 'f32')):
        return False
    # the schedule for small graphs, decided here on the host from the library's own limits (skf_small_graph_limits) -- not
    # by uploading the graph and binding a plan only to ask skf_plan_batchable, and not from a second copy of the constants
    from ..._engine import small_graph_limits
    lim = small_graph_limits()
    graph = fuser.fusion_graph
    types = list(graph.object_types)
    if len(types) > lim['max_types'] or any(int(ot.rank) > lim['max_rank'] for ot in types):
        return False
    n_rel = n_theta = 0
    for rel in graph.relations:
        if max(rel.data.shape) > lim['max_objects']:
            return False
        if rel.row_type is rel.col_type:
            n_theta += 1
            n = rel.data.shape[0]
            if rel.is_zero_unstored():          # counted on the sparse matrix itself, never expanded
                nnz = int(rel.constraint_entries().known)
            else:
                nnz = int(np.count_nonzero(np.ma.getdata(rel.dense_data())))
            if nnz == 0 or nnz > n * n // lim['constraint_nnz_divisor']:
                return False
        else:
            n_rel += 1
    return 1 <= n_rel <= lim['max_relations'] and n_theta <= lim['max_constraints']


def store_runs(fuser, runs):
    """(G, S) per run -> factors_[object_type][run], backbones_[relation][run]
    (dfmf.py:97-105)."""
    fuser.factors_ = defaultdict(list)
    fuser.backbones_ = defaultdict(list)
    graph = fuser.fusion_graph
    for G, S in runs:
        for (object_type, _), factor in G.items():
            fuser.factors_[object_type].append(factor)
        for (row_type, col_type), backbones in S.items():
            for k, relation in enumerate(graph.get_relations(row_type, col_type)):
                fuser.backbones_[relation].append(backbones[k])


def _relation_name(relation):
    return 'R_(%s,%s)' % (relation.row_type.name, relation.col_type.name)


def heldout_lists(fuser):
    """`validation` = [(relation, heldout)] of a fuser -> the lists of `_dfmf.Validation`: [(((row_type, col_type), l), rows,
    cols, values)], l the relation's position among the graph's relations of its pair.  `heldout`: a scipy.sparse matrix
    of the relation's shape whose STORED entries are the held-out pairs with their true values, or (rows, cols, values).
    Refused, naming the relation (DataFusionError: not in the graph; ValueError: the rest): a constraint, a preprocessor
    on the relation, a shard other than 'runs', two lists for one relation, no pair at all, an index out of range, a value
    that is not finite, and a held-out pair the training relation KNOWS -- a stored entry of a scipy.sparse relation with
    ``unstored='unknown'``, an unmasked cell of a MaskedArray: validation data leaking into training.  Plain arrays and
    ``unstored='zero'`` relations have no notion of an unknown cell and are accepted as they are."""
    from ..base import DataFusionError
    import scipy.sparse
    graph = fuser.fusion_graph
    if fuser.shard != 'runs':
        raise ValueError("validation needs shard='runs' (a whole fit on this process), not shard=%r" % (fuser.shard,))
    out, seen = [], []
    for item in fuser.validation:
        relation, held = item
        if not any(relation is r for r in graph.relations):
            raise DataFusionError('validation: relation %s is not in the fusion graph' % _relation_name(relation))
        name = _relation_name(relation)
        if relation.row_type == relation.col_type:
            raise ValueError('validation: %s is a constraint, not a relation between two object types' % name)
        if relation.preprocessor:
            raise ValueError('validation: %s has a preprocessor: held-out values would be compared with preprocessed data' % name)
        if any(relation is r for r in seen):
            raise ValueError('validation: two held-out lists for %s' % name)
        seen.append(relation)
        if scipy.sparse.issparse(held):
            if tuple(held.shape) != tuple(relation.data.shape):
                raise ValueError('validation: held-out matrix of %s has shape %r, the relation %r'
                                 % (name, tuple(held.shape), tuple(relation.data.shape)))
            coo = scipy.sparse.coo_matrix(held)
            rows, cols, vals = coo.row, coo.col, coo.data
        else:
            rows, cols, vals = held
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        cols = np.asarray(cols, dtype=np.int64).reshape(-1)
        vals = np.asarray(vals, dtype=np.float64).reshape(-1)
        if not (rows.size == cols.size == vals.size) or rows.size == 0:
            raise ValueError('validation: %s needs rows, cols and values of one length, at least one pair' % name)
        n_r, n_c = relation.data.shape
        if rows.min() < 0 or rows.max() >= n_r or cols.min() < 0 or cols.max() >= n_c:
            raise ValueError('validation: a held-out pair of %s lies outside its %d x %d entries' % (name, n_r, n_c))
        if not np.isfinite(vals).all():
            raise ValueError('validation: a held-out value of %s is not finite' % name)
        known = None
        if relation.is_known_entries():
            csr = scipy.sparse.csr_matrix(relation.data)
            pattern = scipy.sparse.csr_matrix((np.ones(csr.indices.size, dtype=np.int8), csr.indices, csr.indptr), shape=csr.shape)
            known = np.asarray(pattern[rows, cols]).reshape(-1) != 0
        elif np.ma.isMaskedArray(relation.data):
            known = ~np.ma.getmaskarray(relation.data)[rows, cols]
        if known is not None and known.any():
            raise ValueError('validation: %d held-out pairs of %s are known to the training relation (validation data leaks '
                             'into training)' % (int(np.count_nonzero(known)), name))
        order = np.lexsort((cols, rows))                # by row, then column: one list whatever order the pairs came in
        rows, cols, vals = rows[order], cols[order], vals[order]
        pair = (relation.row_type, relation.col_type)
        l = [k for k, r in enumerate(graph.get_relations(*pair)) if r is relation][0]
        out.append(((pair, l), rows, cols, vals))
    if not out:
        raise ValueError('validation: no held-out list given')
    return out


def _new_validation(fuser, lists):
    return _dfmf.Validation(lists, patience=fuser.patience, min_delta=fuser.min_delta, check_every=fuser.check_every,
                            restore_best=fuser.restore_best)


def store_validation(fuser, per_run):
    """What the monitors of the restarts left behind -> per-run attributes, as factors_ / backbones_ are kept:
    validation_sqerr_[run] (iterations x lists), validation_rmse_[run] (pooled over the lists, per iteration),
    best_iter_[run], n_iter_[run], stopped_early_[run]; all None for a fit without `validation`."""
    if per_run is None:
        fuser.validation_sqerr_ = fuser.validation_rmse_ = fuser.best_iter_ = fuser.n_iter_ = fuser.stopped_early_ = None
        return
    pairs = float(sum(v[1].size for v in per_run[0].lists))
    fuser.validation_sqerr_ = [v.sqerr for v in per_run]
    fuser.validation_rmse_ = [np.sqrt(v.sqerr.sum(axis=1) / pairs) for v in per_run]
    fuser.best_iter_ = [int(v.best_iter) for v in per_run]
    fuser.n_iter_ = [int(v.n_iter) for v in per_run]
    fuser.stopped_early_ = [bool(v.stopped) for v in per_run]


class _Fuser(FusionFit):
    """`fuse` of ``Dfmf`` and ``Dfmc``: one implementation; the class attributes say what differs."""

    _variant = None             # 'dfmf' | 'dfmc': which update rules, and the variant the `*_apply` rules decide for
    _keeps_masks = False        # what is still masked after fill + preprocess is unknown and completed by the model
    _takes_known_entries = False    # a relation given as its known entries may enter as such (shard 'runs' / 'owned')
    _shares_launches = False    # restarts of a small graph may share their launches, whatever n_jobs says

    def _solve(self, M, **kw):
        """One restart through the functional seam of the variant."""
        raise NotImplementedError

    def fuse(self, fusion_graph):
        from ... import _native as nat
        self.fusion_graph = fusion_graph
        validation = getattr(self, 'validation', None)
        if validation is None and getattr(self, 'patience', None) is not None:
            raise ValueError('patience without validation: early stopping on held-out pairs needs the pairs')
        lists = heldout_lists(self) if validation is not None else None
        if lists is not None:
            _new_validation(self, lists)                # (the parameter checks, before anything is uploaded)
        store_validation(self, None)
        self.random_state = _random_state(self.random_state)
        object_types = list(fusion_graph.object_types)
        rank = {ot: int(ot.rank) for ot in object_types}
        matrices = graph_matrices(fusion_graph, with_masks=self._keeps_masks, device_dtype=device_fill_dtype(self),
                                  known_entries=self._takes_known_entries and self.shard in ('runs', 'owned'),
                                  sparse_relations=getattr(self, 'sparse_relations', None), shard=self.shard,
                                  sparse_constraints=getattr(self, 'sparse_constraints', None), variant=self._variant)
        R, Theta, M = matrices if self._keeps_masks else matrices + (None,)
        self.init_on_device_ = init_device_wanted(self) and init_device_covered(R, M)
        G0 = initial_factors(R, object_types, rank, self.init_type, self.random_state, self.n_run, self.init_on_device_)
        kw = dict(R=R, Theta=Theta, obj_types=object_types, obj_type2rank=rank,
                  max_iter=self.max_iter, init_type=self.init_type, stopping=self.stopping,
                  stopping_system=self.stopping_system, verbose=self.verbose,
                  compute_err=self.compute_err, callback=self.callback,
                  random_state=self.random_state, n_jobs=self.n_jobs, dtype=self.dtype)
        code = {'dfmf': nat.SKF_DFMF, 'dfmc': nat.SKF_DFMC}[self._variant]
        if lists is not None:
            # every restart is monitored on its own, one after the other: the shared-launch and concurrent paths are for
            # the plain loop (as with a callback)
            monitors = {k: _new_validation(self, lists) for k in my_runs(self.n_run)}
            local = {k: self._solve(M, G0=G0[k], validation=monitors[k], **kw) for k in monitors}
            store_runs(self, gather_runs(local, self.n_run))
            store_validation(self, [monitors[k] for k in range(self.n_run)] if len(monitors) == self.n_run else None)
            return self
        if self.shard in ('relations', 'rows', 'owned'):                   # all GPUs cooperate on every restart
            # (an owned fit takes the constraints graph_matrices left as entries: each rank the slice of its owned rows)
            store_runs(self, [self._solve(M, G0=G0[k], shard=self.shard, sparse_constraints=self.shard == 'owned', **kw)
                              for k in range(self.n_run)])
            return self
        if self._shares_launches and shared_launches(self):
            runs = _dfmf.run_fits_concurrent(code, R, M, Theta, object_types, rank, self.max_iter, self.dtype,
                                             G0, None, min(self.n_run, 32), batch_only=True)
            if runs is not None:
                store_runs(self, runs)
                return self
        n_streams = concurrent_streams(self)
        if n_streams:                                   # n_jobs restarts side by side on this GPU
            store_runs(self, _dfmf.run_fits_concurrent(code, R, M, Theta, object_types, rank,
                                                       self.max_iter, self.dtype, G0, None, n_streams))
            return self
        local = {k: self._solve(M, G0=G0[k], **kw)
                 for k in my_runs(self.n_run)}          # one restart per GPU when distributed
        store_runs(self, gather_runs(local, self.n_run))
        return self


class Dfmf(_Fuser):
    """Data fusion by matrix factorization.

    Parameters (identical to the reference): max_iter=100, init_type='random_c', n_run=1,
    stopping=None, stopping_system=None, verbose=0, compute_err=False, callback=None,
    random_state=None, n_jobs=1 (here: that many restarts run concurrently on streams of one GPU;
    results do not depend on it).  Additions: dtype='f64' | 'f32' | 'bf16' (device arithmetic),
    shard='runs' | 'relations' | 'rows' | 'owned' (what a torch.distributed process group shares out: whole
    restarts -- no collective; the relations of each restart -- one all-reduce per iteration;
    balanced row blocks of the relations -- all-reduces of W, Q and E / D per iteration; or the rows of
    every object type with the matching rows of its relations -- a reduce-scatter of each partial Q and an
    all-gather of the updated factor rows, the form with the least exchange).
    sparse_relations=None | True | False: a ``scipy.sparse`` relation (``unstored='zero'``) is fitted on its stored entries
    alone, never expanded, with shard='runs' or shard='owned' (every rank then uploads the CSR of its owned rows only and no
    dense row block exists anywhere; each process still holds the whole scipy.sparse matrix on the host, which the
    initialisers read), no preprocessor and two different object
    types -- None: when
    density * max(rank_row, rank_col) <= 4 and the relation is beyond the small-graph limits (a rank above 64 or more
    than 8192 objects on a side); True: always; False: never (``toarray()``).
    sparse_constraints=None | True | False: a ``scipy.sparse`` constraint (a relation of a type with itself,
    ``unstored='zero'``) goes to the device as its entries, never expanded, with shard='runs' or shard='owned' (every rank
    then hands over the CSR of its owned rows over all columns; no rank holds the whole constraint on its device) and no
    preprocessor -- None:
    when nnz <= n * n / 16 (the engine's own bound for the sparse product; a denser one is expanded and multiplied as a
    dense matrix); True: always; False: never (``toarray()``).  Same factors either way, bit for bit, up to that bound.
    A ``scipy.sparse`` relation with MISSING values (``Relation(..., unstored='unknown')``, any ``fill_value``) is fitted
    as entries plus rank one under the same ``sparse_relations`` rule with shard='runs' and never expanded either: every
    fill writes a rank-one pattern a b^T into the unknown cells, so the filled matrix is a b^T + D with D sparse on the
    stored pattern (``Relation.filled_entries``; see ``filled_entries_apply`` for what is still expanded).
    init_device=None | True | False: the column means of `random_c` / `random_vcol` (reference _init.py:20-61) are formed on
    the device -- one contraction per relation view against the 0/1 matrix of the chosen columns, the random stream drawn on
    the host exactly as before -- when the fit is eligible (``init_device_wanted``, ``init_device_covered``: shard='runs', no
    preprocessor, the first relation of every pair whole, not a MaskedArray, dense, stored entries, or a relation with missing
    values kept as lists -- there one pass over the lists per view --, at least 5 columns both ways);
    True: whenever eligible; None: when the host initialiser would gather at least 2^34 elements or walk at least 2^33
    entries of relations with missing values; False: never.  An
    ineligible fit initialises on the host whatever this says.  ``init_on_device_`` (after ``fuse``) says what ran.
    ``device_fill=True`` goes with these initialisers when they run on the device.
    validation=None | [(relation, heldout)]: held-out pairs scored INSIDE the fit (shard='runs').  `heldout` is a
    ``scipy.sparse`` matrix of the relation's shape whose stored entries are the held-out pairs with their true values, or
    a tuple (rows, cols, values).  After every iteration the device adds up (value - prediction)^2 over every list; the
    criterion is the POOLED sum of squared errors over all lists (one number per iteration, whatever the lists' sizes).
    patience=None | n: n iterations in a row without an improvement (pooled sum < best - min_delta) end the fit;
    check_every=8: iterations issued between two looks at the verdict -- the loop stays on the device, so a fit that stops at
    iteration t runs on to the next multiple, but history, best iterate and model do not depend on it.
    restore_best=True: ``factor()`` / ``backbone()`` are the best iterate (a device copy taken when it was judged); False:
    the last.  After ``fuse``, per run: ``validation_sqerr_`` (iterations x lists, up to the stop), ``validation_rmse_``
    (pooled), ``best_iter_`` (1-based), ``n_iter_``, ``stopped_early_``; all None without `validation`.  Restarts are
    monitored one after the other.  See ``heldout_lists`` for what is refused (a held-out pair the training relation knows
    among them).
    """

    _variant = 'dfmf'
    _shares_launches = True

    def __init__(self, max_iter=100, init_type='random_c', n_run=1, stopping=None,
                 stopping_system=None, verbose=0, compute_err=False, callback=None,
                 random_state=None, n_jobs=1, dtype='f64', shard='runs', device_fill=False, sparse_relations=None,
                 sparse_constraints=None, init_device=None, validation=None, patience=None, min_delta=0.0, check_every=8,
                 restore_best=True):
        super(Dfmf, self).__init__()
        self._set_params(vars())

    def _solve(self, M, **kw):
        return _dfmf.dfmf(**kw)


class DfmfTransform(FusionTransform):
    """Online transformer of new objects into a fitted fused space.

    Parameters (identical to the reference): max_iter=100, init_type=None (use the fuser's),
    n_run=1, stopping=None, stopping_system=None, fill_value=0, verbose=0, compute_err=False,
    callback=None, random_state=None, n_jobs=1.  Additions: dtype;
    sparse_relations=None | True | False: a new ``scipy.sparse`` relation (``unstored='zero'``, no preprocessor, two
    different object types, ranks <= 1024) enters as its stored entries compressed along the target's side and is never
    expanded -- True: whenever eligible; False: never (``toarray()``); None: when density * max(rank) <= 4 and the relation
    has at least 2^20 cells (below that the dense upload is free and results stay bit for bit).  Stored non-finite values
    take `fill_value`, as in the dense path; entries that are not stored are zeros, not unknowns, and never filled.  A
    relation given with ``unstored='unknown'`` is still expanded: the reference's fold-in fills it (``DfmcTransform`` folds
    new objects in on their known entries alone).
    sparse_constraints=None | True | False: a ``scipy.sparse`` constraint on the target goes to the device as its entries,
    under the rule of ``Dfmf``.
    """

    def __init__(self, max_iter=100, init_type=None, n_run=1, stopping=None,
                 stopping_system=None, fill_value=0, verbose=0, compute_err=False,
                 callback=None, random_state=None, n_jobs=1, dtype='f64', sparse_relations=None, sparse_constraints=None):
        super(DfmfTransform, self).__init__()
        self._set_params(vars())

    def _enter(self, relation, target, R, Theta):
        """One relation of the new graph into R / Theta (dfmf.py:176-189: preprocess, fill masked / non-finite entries with
        `fill_value`), or as its stored entries where `fold_entries_apply` / `constraint_entries_apply` say so."""
        key = (relation.row_type, relation.col_type)
        if fold_entries_apply(relation, getattr(self, 'sparse_relations', None)):
            # the stored entries, compressed along the target's side; `data[~isfinite] = fill_value` of the dense
            # path on the stored values (what is not stored is zero, not unknown: nothing else to fill)
            data = relation.stored_entries(by_col=relation.row_type != target)
            data.values[~np.isfinite(data.values)] = self.fill_value
            R.setdefault(key, []).append(data)
            return
        if relation.row_type == target and constraint_entries_apply(relation, getattr(self, 'sparse_constraints', None)):
            Theta.setdefault(key, []).append(relation.constraint_entries())
            return
        data = relation.preprocessor(relation.dense_data()) if relation.preprocessor \
            else relation.dense_data()
        if np.ma.is_masked(data):
            data.fill_value = self.fill_value
            data = data.filled()
        data[~np.isfinite(data)] = self.fill_value
        dest = R if relation.row_type != relation.col_type else Theta
        dest.setdefault(key, []).append(data)

    def transform(self, target, fusion_graph, fuser):
        self.target = target
        self.fusion_graph = fusion_graph
        self.fuser = fuser
        self._validate_graph()
        init_type = self.init_type if self.init_type is not None else fuser.init_type
        self.random_state = _random_state(self.random_state)
        rank = {ot: int(ot.rank) for ot in fusion_graph.object_types}

        R, Theta = {}, {}
        for row_type, col_type in product(fusion_graph.object_types, repeat=2):
            for relation in fusion_graph.get_relations(row_type, col_type):
                self._enter(relation, target, R, Theta)

        def frozen_model(run):
            """(G, S) of restart `run` (dfmf.py:109-115); only the LAST relation of a type pair survives in S there --
            kept: one backbone per pair."""
            G = {(ot, ot): fuser.factor(ot, run) for ot in fuser.fusion_graph.object_types}
            S = {(rel.row_type, rel.col_type): [fuser.backbone(rel, run)]
                 for rel in fuser.fusion_graph.relations if rel.row_type != rel.col_type}
            return G, S

        self.factors_ = defaultdict(list)
        if self.n_run > 1 and not (self.callback or self.stopping or self.stopping_system or self.compute_err):
            # the fold-ins into the models of all restarts share the uploads of the new relations and every launch
            # (reference: one joblib task per restart, dfmf.py:191-199)
            self.factors_[target] = _dfmf.transform_runs(R, Theta, target, rank, [frozen_model(run) for run in range(self.n_run)],
                                                         max_iter=self.max_iter, init_type=init_type,
                                                         random_state=self.random_state, dtype=self.dtype)
            return self
        for run in range(self.n_run):
            G, S = frozen_model(run)
            G_new = _dfmf.transform(R_ij=R, Theta_i=Theta, target_obj_type=target,
                                    obj_type2rank=rank, G=G, S=S, max_iter=self.max_iter,
                                    init_type=init_type, stopping=self.stopping,
                                    stopping_system=self.stopping_system, verbose=self.verbose,
                                    compute_err=self.compute_err, callback=self.callback,
                                    random_state=self.random_state, dtype=self.dtype)
            self.factors_[target].append(G_new)
        return self
