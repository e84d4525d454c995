"""Factor initialisers.

They run once per fit, consume a ``numpy.random.RandomState`` (MT19937) stream and must draw
from it in exactly the reference's order for seeded results to agree (reference
``_init.py:6-61``: `random` :11-17, `random_c` :20-41, `random_vcol` :44-61), so the DRAWS stay
on the host.  `initialize` also forms G0 there, in NumPy, and the result is uploaded once;
`draw_positions` / `DeviceInit` make the same draws without the data and leave the column means
of `random_c` / `random_vcol` to the device (csrc/skf_init.h).  ``R`` maps (row_type, col_type)
to the FIRST relation matrix of that pair (reference _dfmf.py:191).
"""
import numpy as np


def host_view(mat):
    """The first relation of a pair as the initialisers read it: a float ndarray, or the relation given as its known
    entries (_engine.KnownEntries) -- whose column statistics are formed from the entries, never from a dense copy."""
    from ..._engine import KnownEntries
    return mat if isinstance(mat, KnownEntries) else np.asarray(mat, dtype=float)


class _KnownView(object):
    """A relation given as its known entries, oriented for one object type (transposed: the type is its column type),
    with the constant `fill` on every entry not stored -- the mask form's data after ``filled()``.  Answers what the
    initialisers ask of a dense view without forming it: its shape, the row means over a set of columns
        sum over a set of entries = sum of the known ones + (unknown ones) * fill
    and every column's 2-norm.  The norms rank the columns in a stable sort, and ratings take few distinct values, so
    columns tie exactly: each norm is taken the reference's way (np.linalg.norm of the dense column, strided as a column
    of the relation is, contiguous as a row is), one column buffer at a time, so that the ties fall as they do there."""

    def __init__(self, ke, transposed):
        self.rows, self.cols = ke.rows_cols()           # (whichever side the lists are compressed along)
        if transposed:
            self.rows, self.cols = self.cols, self.rows
        self.transposed = transposed
        self.shape = ke.shape[::-1] if transposed else ke.shape
        self.values, self.fill = ke.values, ke.fill
        self.zeros = getattr(ke, 'unstored', 'unknown') == 'zero'      # the entries not stored ARE zeros (a scipy.sparse relation)
        # a per-line fill (a filled relation with missing values): an entry not stored holds a[row] * b[column] in the
        # view's orientation; one of the two is all ones, so the product is the dense fill value bit for bit
        self.a = self.b = None
        if getattr(ke, 'row_fill', None) is not None:
            self.a, self.b = (ke.col_fill, ke.row_fill) if transposed else (ke.row_fill, ke.col_fill)
            self.zeros = False

    def row_means(self, columns):
        if self.zeros:
            # bit for bit the dense statement: ``view[:, columns]`` comes out column-major, its ``mean(axis=1)`` adds the
            # chosen columns one after the other in the order drawn, and adding a zero changes nothing -- so the stored
            # entries of every row are added in the order their columns were drawn
            pos = np.full(self.shape[1], -1, dtype=np.int64)
            pos[columns] = np.arange(len(columns))
            at = pos[self.cols]
            hit = np.nonzero(at >= 0)[0]
            hit = hit[np.argsort(at[hit], kind='stable')]
            return np.bincount(self.rows[hit], weights=self.values[hit], minlength=self.shape[0]) / len(columns)
        sel = np.zeros(self.shape[1], dtype=bool)
        sel[columns] = True
        hit = sel[self.cols]
        known = np.bincount(self.rows[hit], weights=self.values[hit], minlength=self.shape[0])
        count = np.bincount(self.rows[hit], minlength=self.shape[0])
        take = len(columns)
        if self.a is not None:      # (known + a_r (sum of b over the chosen columns - sum of b over the stored chosen ones)) / take
            b_stored = np.bincount(self.rows[hit], weights=self.b[self.cols[hit]], minlength=self.shape[0])
            return (known + self.a * (self.b[columns].sum() - b_stored)) / take
        return (known + (take - count) * self.fill) / take

    def column_norms(self):
        order = np.argsort(self.cols, kind='stable')
        ptr = np.zeros(self.shape[1] + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.cols, minlength=self.shape[1]), out=ptr[1:])
        rows, vals = self.rows[order], self.values[order]
        col = np.empty(self.shape[0]) if self.transposed else np.empty((self.shape[0], 2))[:, 0]
        norms = []
        for k in range(self.shape[1]):
            col[:] = self.fill if self.a is None else self.a * self.b[k]
            col[rows[ptr[k]:ptr[k + 1]]] = vals[ptr[k]:ptr[k + 1]]
            norms.append(np.linalg.norm(col, 2))
        return norms


def _views_of(obj_type, R):
    """Every relation that touches obj_type, oriented so that its rows are obj_type's objects, with a key that names the
    oriented view ((pair, transposed?))."""
    from ..._engine import KnownEntries
    for pair, mat in R.items():
        if obj_type in pair:
            if isinstance(mat, KnownEntries):
                yield _KnownView(mat, obj_type != pair[0]), (pair, obj_type != pair[0])
                continue
            yield (mat if obj_type == pair[0] else mat.T), (pair, obj_type != pair[0])


def _random(obj_types, n_obj, rank, R, random_state):
    return {(t, t): random_state.rand(n_obj[t], rank[t]) for t in _ordered(obj_types)}


def _ordered(obj_types):
    # iteration order of the caller's container == RNG consumption order
    return list(obj_types)


def _column_means_init(obj_types, n_obj, rank, R, random_state, pool_of):
    """G_t = 1e-5 + sum over relations of |mean of p randomly chosen columns| per factor column.
    ``pool_of(view)`` returns the column index pool that is shuffled before every draw."""
    G = {}
    for t in _ordered(obj_types):
        c = rank[t]
        acc = np.full((n_obj[t], c), 1e-5)
        for view, key in _views_of(t, R):
            n_cols = view.shape[1]
            take = int(.2 * n_cols)
            pool = pool_of(view, key)
            part = np.zeros((n_obj[t], c))
            for k in range(c):
                random_state.shuffle(pool)
                if isinstance(view, _KnownView):
                    part[:, k] = view.row_means(pool[:take])
                else:
                    part[:, k] = view[:, pool[:take]].mean(axis=1)
            acc += np.abs(part)
        G[t, t] = acc
    return G


def _random_vcol(obj_types, n_obj, rank, R, random_state):
    return _column_means_init(obj_types, n_obj, rank, R, random_state,
                              lambda view, key: np.arange(view.shape[1]))


def _random_c(obj_types, n_obj, rank, R, random_state, pools=None):
    # `pools`: {(type pair of the relation, transposed?): the strongest half of its columns} kept by the caller across the
    # restarts of ONE fit -- the ranking by column norm draws nothing from the random stream and the matrices do not change
    # between restarts, yet at n_run = 10 on the README graph it was 9 of the 17 ms the ten initialisations took (3 800
    # norm calls).  Every call still starts from a FRESH copy of the ranked list, as the reference builds it anew.
    def strongest_half(view, key):
        if pools is not None and key in pools:
            return list(pools[key])
        n_cols = view.shape[1]
        if isinstance(view, _KnownView):
            norms = view.column_norms()
        else:
            norms = [np.linalg.norm(view[:, k], 2) for k in range(n_cols)]
        order = sorted(range(n_cols), key=norms.__getitem__, reverse=True)   # stable, descending
        half = order[:int(.5 * n_cols)]
        if pools is not None:
            pools[key] = tuple(half)
        return half
    return _column_means_init(obj_types, n_obj, rank, R, random_state, strongest_half)


INIT_TYPES = {"random": _random, "random_c": _random_c, "random_vcol": _random_vcol}
COLUMN_MEAN_TYPES = ('random_c', 'random_vcol')


# ---- the column-mean initialisers on the device ------------------------------------------------------------------------------
# `RandomState.shuffle` makes the same draws and the same swaps whatever the sequence holds, so the host can shuffle an index
# array arange(len(pool)) cumulatively exactly where `_column_means_init` shuffles the pool, without knowing what the pool
# holds: the chosen columns are pool0[idx[:take]] and the stream is consumed as before.  What needs the data -- the column
# norms that rank the pool of `random_c`, the means themselves -- runs on the device (csrc/skf_init.h).

def draw_positions(obj_types, obj_type2rank, shapes, init_typ, random_state):
    """The random draws of one `initialize` call with a column-mean initialiser, without the data: for every object type
    (in the caller's order) and every oriented view of it (in the order of `_views_of`) the c x take positions into the
    view's column pool -- ``{type: [((pair, transposed?), int64 array c x take)]}``.  `shapes`: {(row_type, col_type):
    (n_row, n_col)} of the FIRST relation of every pair, in the order of R.  The pool of `random_vcol` is every column of
    the view, so its positions are the columns themselves; `random_c` draws from the strongest half (`DeviceInit`)."""
    if init_typ not in COLUMN_MEAN_TYPES:
        raise KeyError(init_typ)
    out = {}
    for t in _ordered(obj_types):
        c = obj_type2rank[t]
        views = []
        for pair, shape in shapes.items():
            if t not in pair:
                continue
            transposed = t != pair[0]
            n_cols = int(shape[0] if transposed else shape[1])
            take = int(.2 * n_cols)
            idx = np.arange(int(.5 * n_cols) if init_typ == 'random_c' else n_cols)
            pos = np.empty((c, take), dtype=np.int64)
            for k in range(c):
                random_state.shuffle(idx)
                pos[k] = idx[:take]
            views.append(((pair, transposed), pos))
        out[t] = views
    return out


def strongest_half_of(squares):
    """The pool of `random_c` from the sums of squares of a view's columns: the square roots ranked by the stable descending
    sort of `_random_c`, so that exact sums tie exactly as the reference's norms do."""
    norms = np.sqrt(np.asarray(squares, dtype=np.float64))
    order = sorted(range(len(norms)), key=norms.__getitem__, reverse=True)
    return np.asarray(order[:int(.5 * len(norms))], dtype=np.int64)


class DeviceInit(object):
    """What stands in for the G0 of one restart when its plan initialises itself on the device: the positions drawn for
    this restart and `pools`, the dict the restarts of ONE fit share -- {(pair, transposed?): strongest half}, filled from the
    device norms by the first plan that needs them, as `pools` of `_random_c` is filled by the first restart."""

    def __init__(self, positions, init_typ, pools):
        self.positions, self.init_typ, self.pools = positions, init_typ, pools

    def _pool(self, plan, rel, key):
        if key not in self.pools:
            row_sq, col_sq = plan.relation_norms(rel)           # (one pass gives both orientations)
            self.pools[key[0], False] = strongest_half_of(col_sq)
            self.pools[key[0], True] = strongest_half_of(row_sq)
        return self.pools[key]

    def apply(self, plan, obj_types):
        """Initialise every factor of the bound `plan`: the selections go up, the plan forms G0 and takes it as its
        factor.  Between bind and the first iteration; one synchronisation at the end."""
        first = {}
        for k, rel in enumerate(plan.relations):
            first.setdefault((rel[0], rel[1]), k)               # the FIRST relation of a pair (reference _dfmf.py:191)
        for t in obj_types:
            views = []
            for key, pos in self.positions[t]:
                rel = first[key[0]]
                views.append((rel, self._pool(plan, rel, key)[pos] if self.init_typ == 'random_c' else pos))
            plan.init_column_means(t, views, sync=False)
        plan.synchronize()
        plan._pending_init = None                               # (selections, scratch and G0 buffers: the launches are through)


def initialize(obj_types, obj_type2n_obj, obj_type2rank, R, init_typ, random_state, pools=None):
    """Unknown ``init_typ`` raises KeyError like the reference dispatcher (_init.py:7-8).  `pools` (optional, a dict the
    caller keeps for the restarts of one fit): see `_random_c`."""
    if init_typ == 'random_c' and pools is not None:
        return _random_c(obj_types, obj_type2n_obj, obj_type2rank, R, random_state, pools)
    return INIT_TYPES[init_typ](obj_types, obj_type2n_obj, obj_type2rank, R, random_state)
