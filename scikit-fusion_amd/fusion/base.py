"""Result accessors shared by the fusers (host side, pure Python).

Mirrors the behaviour of reference ``skfusion/fusion/base/base.py``:
``factor`` (:35-56), ``backbone`` (:169-189), ``complete`` (:119-146), ``chain`` (:69-96),
``FusionTransform._validate_graph`` (:224-231) and ``DataFusionError`` (:250), including the
"generator when n_run > 1 and run is None" convention.
"""
from collections import defaultdict

import numpy as np

__all__ = ['FusionBase', 'FusionFit', 'FusionTransform', 'DataFusionError', 'save_fit', 'load_fit']


class DataFusionError(Exception):
    """API misuse: unknown object type / relation, inconsistent graph."""


class FusionBase(object):
    """Holds the constructor parameters and the fitted factors of all runs.

    ``factors_[object_type][run]`` and ``backbones_[relation][run]`` are filled by the
    concrete fusers.
    """
    _params = None

    def __init__(self):
        self.factors_ = defaultdict(list)
        self.backbones_ = defaultdict(list)

    def _set_params(self, values):
        # `values` is the vars() of the subclass constructor (reference base.py:29-33)
        self._params = {k: v for k, v in values.items() if k not in ('self', '__class__')}
        self.__dict__.update(self._params)

    # one run -> the matrix; several runs and no explicit run -> an iterator over runs
    def _select(self, per_run, run):
        if self.n_run > 1 and run is None:
            return (per_run[k] for k in range(self.n_run))
        return per_run[0 if run is None else run]

    def factor(self, object_type, run=None):
        """Latent factor G of ``object_type`` (n_objects x rank)."""
        if object_type not in self.fusion_graph.object_types:
            raise DataFusionError("Object type %s is not included in the fusion scheme"
                                  % object_type.name)
        if object_type not in self.factors_:
            raise DataFusionError("Unknown object type.")
        return self._select(self.factors_[object_type], run)

    def chain(self, row_type, col_type):
        """All simple paths row_type -> ... -> col_type along relation directions
        (breadth first, shortest first), as lists of object types."""
        frontier = [[row_type]]
        if row_type == col_type:
            yield frontier[0]
        while frontier:
            nxt = []
            for path in frontier:
                for ot in self.fusion_graph.out_neighbors(path[-1]):
                    if ot in path:
                        continue
                    longer = path + [ot]
                    if ot == col_type:
                        yield longer
                    else:
                        nxt.append(longer)
            frontier = nxt

    # ---- chained latent profiles on the device --------------------------------------------------------
    # The reference's base.py:69-96 only enumerates the paths; what its users compute from them is, per path c,
    #     bb = reduce(np.dot, [backbone(first relation c[i] -> c[i+1])])          (examples/dicty_chaining.py:43-45)
    #     profile = G_row . bb . G_col^T        (dicty_chaining.py:46-49)    or    G_row . bb   (pharma_chaining.py:48-50)
    # hstack-ed over the object types and their paths (the path [row_type] contributes G_row itself).  At BASELINE config-3
    # sizes one such block is 50k x 100k: it is produced blockwise on the device like `complete_blocks`.
    def _chain_source(self, row_type, run):
        """(the fit whose backbones / column factors the paths use, the factor of the starting type in run `run`)"""
        raise NotImplementedError

    def chain_paths(self, row_type, col_types=None, skip=()):
        """[(col_type, path)] in the order the reference examples walk them: object types in `col_types` order (default:
        the graph's), the paths of `chain()` for each, types in `skip` left out."""
        fit, _ = self._chain_source(row_type, 0)
        cols = list(fit.fusion_graph.object_types) if col_types is None else list(col_types)
        out = []
        for ct in cols:
            if any(ct is s or ct == s for s in skip):
                continue
            for path in FusionBase.chain(fit, row_type, ct):      # the FITTED model's graph, also for a transformer
                out.append((ct, path))
        return out

    def chain_backbone(self, path, run=None):
        """Product of the backbones of the FIRST relation of every hop of `path` (as the examples take them), reduced on
        the device in f64 (`_engine.chain_backbone`); None for the one-type path."""
        from .._engine import chain_backbone
        run = 0 if run is None else run
        fit, _ = self._chain_source(path[0], run)
        hops = []
        for a, b in zip(path[:-1], path[1:]):
            rels = list(fit.fusion_graph.get_relations(a, b))
            if not rels:
                raise DataFusionError("No relation %s -> %s on the path" % (a.name, b.name))
            hops.append(fit.backbone(rels[0], run))
        return chain_backbone(hops) if hops else None

    def chain_profile_blocks(self, row_type, col_types=None, block_rows=4096, run=None, dtype='f64', project=True,
                             skip=()):
        """Yields ``(row_slice, X[row_slice])``: the chained latent profile of the objects of ``row_type`` (for a
        transformer: of its target's NEW objects), at most ``block_rows`` rows at a time -- for every path of
        ``chain_paths`` the block ``G_row[rows] . (prod of backbones) . G_col^T`` (``project=True``, reference
        examples/dicty_chaining.py:40-53) or ``G_row[rows] . (prod of backbones)`` (``project=False``,
        pharma_chaining.py:43-53), the one-type path contributing ``G_row[rows]`` itself, hstack-ed in path order.  The
        backbone products (f64) and the column factors are uploaded once and stay resident across the blocks; the two
        GEMMs of a block run in the master type of ``dtype`` ('f64' | 'f32' | 'bf16' -> f32).  float64 ndarrays."""
        from .._engine import DeviceReconstructor
        run = 0 if run is None else run
        fit, G_row = self._chain_source(row_type, run)
        for who in {id(self): self, id(fit): fit}.values():          # (a transformer and the fitted model it folds into)
            if not 0 <= int(run) < int(getattr(who, 'n_run', 1)):
                raise DataFusionError("run %d requested, %s holds %d" % (run, type(who).__name__, getattr(who, 'n_run', 1)))
        G_row = np.asarray(G_row)
        parts, col_on_device = [], {}             # one uploaded copy of a column factor, however many paths end in its type
        for ct, path in self.chain_paths(row_type, col_types, skip):
            bb = self.chain_backbone(path, run)
            if bb is None:
                parts.append(None)
            else:
                rec = DeviceReconstructor(bb, fit.factor(ct, run) if project else None, dtype=dtype,
                                          G_col_device=col_on_device.get(ct))
                if project:
                    col_on_device.setdefault(ct, rec.b)
                parts.append(rec)
        if not parts:
            raise DataFusionError("No path from %s to the requested object types" % row_type.name)
        for r0 in range(0, G_row.shape[0], int(block_rows)):
            sl = slice(r0, min(r0 + int(block_rows), G_row.shape[0]))
            rows = G_row[sl]
            yield sl, np.hstack([np.asarray(rows, dtype=np.float64) if rec is None else rec.block(rows) for rec in parts])

    def chain_profile(self, row_type, col_types=None, run=None, dtype='f64', project=True, skip=(), block_rows=4096):
        """The whole profile matrix (``np.vstack`` of ``chain_profile_blocks``) -- for sizes that fit the host."""
        return np.vstack([blk for _, blk in self.chain_profile_blocks(row_type, col_types, block_rows, run, dtype,
                                                                      project, skip)])

    def __repr__(self):
        inner = ', '.join('{}={}'.format(k, v) for k, v in (self._params or {}).items())
        return '{}({})'.format(type(self).__name__, inner)

    __str__ = __repr__


class FusionFit(FusionBase):
    """Accessors of a fitted fuser: backbones and reconstructed relations."""

    def _chain_source(self, row_type, run):
        return self, self.factor(row_type, run)

    def backbone(self, relation, run=None):
        """Backbone S of ``relation`` (rank_row x rank_col)."""
        types = self.fusion_graph.object_types
        if relation.row_type not in types or relation.col_type not in types:
            raise DataFusionError('Object types are not recognized.')
        if relation not in self.backbones_:
            raise DataFusionError("Unknown relation.")
        return self._select(self.backbones_[relation], run)

    def _reconstruct(self, relation, run):
        G1 = self.factor(relation.row_type, run)
        S12 = self.backbone(relation, run)
        G2 = self.factor(relation.col_type, run)
        approx = np.dot(G1, np.dot(S12, G2.T))
        if relation.postprocessor:
            approx = relation.postprocessor(approx)
        return approx

    def complete(self, relation, run=None):
        """Reconstructed relation ``G_row S G_col^T`` (post-processed if the relation has a
        postprocessor)."""
        types = self.fusion_graph.object_types
        if relation.row_type not in types or relation.col_type not in types:
            raise DataFusionError("Object type %s or %s are not included in the fusion scheme"
                                  % (relation.row_type.name, relation.col_type.name))
        if self.n_run > 1 and run is None:
            return (self._reconstruct(relation, k) for k in range(self.n_run))
        return self._reconstruct(relation, 0 if run is None else run)


    def save(self, path):
        """Write the fitted model to ``path`` (one ``.npz``; see ``save_fit``)."""
        return save_fit(self, path)

    @staticmethod
    def load(path, fusion_graph=None):
        """Read a model written by ``save`` (see ``load_fit``)."""
        return load_fit(path, fusion_graph)

    def complete_blocks(self, relation, block_rows=4096, run=None, dtype='f64', device=False):
        """Blockwise reconstruction on the device: yields ``(row_slice, R_hat[row_slice])`` with
        at most ``block_rows`` rows per block, so that a relation whose dense reconstruction is too
        large for the host (BASELINE config 3: up to 40 GB) can be consumed piece by piece.  The backbone and the
        column factor are uploaded once and stay resident in HBM across the blocks.  ``device=True`` yields the
        block as a device-resident matrix in the engine's MASTER type (f64 for ``dtype='f64'``, f32 for ``'f32'`` and
        ``'bf16'``) that aliases a scratch buffer: it is valid until the next block and is NOT post-processed -- a
        relation with a postprocessor is refused with ``device=True``; otherwise a float64 ndarray, post-processed
        per block (exact for element-wise postprocessors).
        Extension of the reference API (``complete`` itself is unchanged)."""
        from .._engine import DeviceReconstructor
        if device and relation.postprocessor:
            raise DataFusionError("complete_blocks(device=True) yields raw device blocks; relation %s -> %s has a "
                                  "postprocessor (use device=False, or apply it to the blocks yourself)"
                                  % (relation.row_type.name, relation.col_type.name))
        run = 0 if run is None else run
        G1 = self.factor(relation.row_type, run)
        rec = DeviceReconstructor(self.backbone(relation, run), self.factor(relation.col_type, run), dtype=dtype)
        for r0 in range(0, G1.shape[0], int(block_rows)):
            sl = slice(r0, min(r0 + int(block_rows), G1.shape[0]))
            block = rec.block(G1[sl], device=device)
            if relation.postprocessor and not device:
                block = relation.postprocessor(block)
            yield sl, block

    # ---- predictions at given pairs and the k best columns of a row, on the device, never densified ----------------------
    # The reference answers both from the dense product (base.py:119-146; examples/movielens_completion.py:121-126 reads
    # R12_pred[hidden]); here nothing of size n_i x n_j is formed on the host or in HBM (`_engine.DeviceCompleter`).
    def _check_relation_types(self, relation):
        types = self.fusion_graph.object_types
        if relation.row_type not in types or relation.col_type not in types:
            raise DataFusionError("Object type %s or %s are not included in the fusion scheme"
                                  % (relation.row_type.name, relation.col_type.name))

    def _check_raw_scores(self, relation, method):
        """The preamble of the operators that rank or compare raw device scores (``method``: the caller's own name)."""
        self._check_relation_types(relation)
        if relation.postprocessor:
            raise DataFusionError("%s ranks raw device scores; relation %s -> %s has a "
                                  "postprocessor (rank complete_blocks(device=False) yourself)"
                                  % (method, relation.row_type.name, relation.col_type.name))

    def _relation_shape(self, relation):
        return np.shape(self.factor(relation.row_type, 0))[0], np.shape(self.factor(relation.col_type, 0))[0]

    @staticmethod
    def _row_vector(rows, n_i):
        """``rows`` as a flat integer array inside the relation; None: every row object."""
        rows = np.arange(n_i) if rows is None else np.asarray(rows).reshape(-1)
        if rows.dtype.kind not in 'iu' or (rows.size and (rows.min() < 0 or rows.max() >= n_i)):
            raise DataFusionError("rows must be integers in 0 .. %d" % (n_i - 1))
        return rows

    def _pair_vectors(self, relation, rows, cols):
        """``rows`` / ``cols`` as flat integer arrays of one length inside the relation, and the relation's shape."""
        rows = np.asarray(rows).reshape(-1)
        cols = np.asarray(cols).reshape(-1)
        if rows.shape != cols.shape or rows.dtype.kind not in 'iu' or cols.dtype.kind not in 'iu':
            raise DataFusionError("rows and cols must be integer arrays of one length")
        n_i, n_j = self._relation_shape(relation)
        if rows.size and (rows.min() < 0 or rows.max() >= n_i or cols.min() < 0 or cols.max() >= n_j):
            raise DataFusionError("A pair lies outside the %d x %d relation" % (n_i, n_j))
        return rows, cols, n_i, n_j

    # one(run) for the one run asked for; several runs and no explicit run -> a generator over the runs (as `_select`)
    def _per_run(self, one, run):
        if self.n_run > 1 and run is None:
            return (one(r) for r in range(self.n_run))
        return one(0 if run is None else run)

    def _completer(self, relation, run, dtype):
        from .._engine import DeviceCompleter
        return (np.asarray(self.factor(relation.row_type, run)),
                DeviceCompleter(self.backbone(relation, run), self.factor(relation.col_type, run), dtype=dtype))

    def complete_entries(self, relation, rows, cols, run=None, dtype='f64'):
        """Predictions ``complete(relation)[rows, cols]`` at the given pairs (float64 vector) without the reconstruction:
        only the distinct rows of the row factor that ``rows`` names go to the device, the pairs in chunks.  The relation's
        postprocessor is applied to the vector (exact for element-wise postprocessors, as in ``complete_blocks``).  The
        products run in the master type of ``dtype`` ('f64' | 'f32' | 'bf16' -> f32).  ``n_run > 1`` and ``run=None``: a
        generator over the runs.  Extension of the reference API."""
        self._check_relation_types(relation)
        rows, cols, _, _ = self._pair_vectors(relation, rows, cols)

        def one(k):
            G1, comp = self._completer(relation, k, dtype)
            out = comp.entries(G1, rows, cols)
            return relation.postprocessor(out) if relation.postprocessor else out
        return self._per_run(one, run)

    def _exclusion_lists(self, relation, exclude, shape):
        """None, or a function ``rows -> (indptr int64, indices int32)``: the excluded columns of the given rows as CSR
        with strictly ascending columns.  Nothing dense is built beyond a block of a mask the caller already holds."""
        if exclude is None:
            return None
        import scipy.sparse
        if isinstance(exclude, str):
            if exclude != 'known':
                raise DataFusionError("exclude must be None, 'known' or a scipy.sparse matrix, not %r" % (exclude,))
            data = relation.data
            if scipy.sparse.issparse(data):
                exclude = data                      # the stored entries, whatever the unstored ones mean
            elif np.ma.isMaskedArray(data):
                mask = np.ma.getmaskarray(data)

                def from_mask(rows):
                    known = ~mask[rows]
                    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
                    np.cumsum(known.sum(axis=1), out=indptr[1:])
                    return indptr, np.nonzero(known)[1].astype(np.int32)
                return from_mask
            else:
                raise DataFusionError("exclude='known': relation %s -> %s is a plain array, every entry of it is known "
                                      "(give the excluded pairs as a scipy.sparse matrix)"
                                      % (relation.row_type.name, relation.col_type.name))
        if not scipy.sparse.issparse(exclude):
            raise DataFusionError("exclude must be None, 'known' or a scipy.sparse matrix, not %s" % type(exclude).__name__)
        if tuple(exclude.shape) != tuple(shape):
            raise DataFusionError("exclude has shape %r, the relation %r" % (tuple(exclude.shape), tuple(shape)))
        csr = scipy.sparse.csr_matrix(exclude)      # (duplicates of a COO matrix are summed; stored zeros stay entries)
        if not csr.has_sorted_indices:
            csr = csr.sorted_indices()

        def from_csr(rows):
            sub = csr[rows]
            if not sub.has_sorted_indices:
                sub.sort_indices()
            return sub.indptr.astype(np.int64), sub.indices.astype(np.int32)
        return from_csr

    def complete_topk(self, relation, k, rows=None, exclude=None, run=None, dtype='f64', block_rows=8192):
        """``(indices int32 [n, k], scores float64 [n, k])``: for each of ``rows`` (default: every row object; otherwise an
        integer array, results in that order) the ``k`` columns the model ranks highest, best first -- higher score
        first, equal scores by lower column index; slots without a candidate hold ``-1`` / ``-inf``.  ``exclude``: None;
        ``'known'`` -- the relation's own known entries (unmasked entries of a MaskedArray relation, stored entries of a
        scipy.sparse relation of either ``unstored=`` kind); or a scipy.sparse matrix of the relation's shape whose stored
        entries are excluded (any format; converted to CSR with sorted indices, never expanded).  Score tiles are formed and
        selected on the device ``block_rows`` rows at a time; the backbone and the column factor stay resident across the
        blocks.  A relation with a postprocessor is refused: the ranking is that of the raw scores and a ranking of
        post-processed values cannot be promised (``complete_blocks(device=True)`` refuses for the same reason).
        ``1 <= k <= 64``.  ``n_run > 1`` and ``run=None``: a generator over the runs.  Extension of the reference API."""
        self._check_raw_scores(relation, 'complete_topk')
        from .._native import SKF_TOPK_MAX
        k = int(k)
        if not 1 <= k <= SKF_TOPK_MAX:
            raise DataFusionError("k = %d outside 1 .. %d" % (k, SKF_TOPK_MAX))
        n_i, n_j = self._relation_shape(relation)
        rows = self._row_vector(rows, n_i)
        lists = self._exclusion_lists(relation, exclude, (n_i, n_j))
        step = max(1, int(block_rows))

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            idx = np.empty((rows.size, k), dtype=np.int32)
            val = np.empty((rows.size, k), dtype=np.float64)
            for b0 in range(0, rows.size, step):
                blk = rows[b0:b0 + step]
                idx[b0:b0 + step], val[b0:b0 + step] = comp.topk(G1[blk], k, exclude=lists(blk) if lists else None)
            return idx, val
        return self._per_run(one, run)

    def complete_ranks(self, relation, rows, cols, exclude=None, run=None, dtype='f64', block_rows=8192):
        """``int64 [n]``: for every pair ``(rows[e], cols[e])`` its 0-based position in the ranking of its row's columns
        by the model -- the number of columns with a higher score, or an equal score and a lower index, in the order of
        ``complete_topk`` -- which is what Recall@k, MRR, NDCG and AUC of held-out pairs need; ``-1`` where the pair's
        score is NaN.  ``exclude`` (as for ``complete_topk``: None, ``'known'`` or a scipy.sparse matrix of the relation's
        shape) removes COMPETITORS only: a pair that is itself excluded is still ranked.  Pairs may come in any order and
        with duplicates.  The counts are taken on the device over score tiles, ``block_rows`` distinct rows at a time;
        nothing of size ``n_i x n_j`` is formed.  A relation with a postprocessor is refused, as in ``complete_topk``.
        ``n_run > 1`` and ``run=None``: a generator over the runs.  Extension of the reference API."""
        self._check_raw_scores(relation, 'complete_ranks')
        rows, cols, n_i, n_j = self._pair_vectors(relation, rows, cols)
        lists = self._exclusion_lists(relation, exclude, (n_i, n_j))
        step = max(1, int(block_rows))
        # the distinct pairs in (row, column) order are the target CSR over the distinct rows; `back` leads home
        key, back = np.unique(rows.astype(np.int64) * n_j + cols.astype(np.int64), return_inverse=True)
        prow, pcol = key // max(n_j, 1), (key % max(n_j, 1)).astype(np.int32)
        urows, first = np.unique(prow, return_index=True)
        ptr = np.append(first, key.size).astype(np.int64)

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            out = np.empty(key.size, dtype=np.int64)
            for b0 in range(0, urows.size, step):
                blk = urows[b0:b0 + step]
                p = ptr[b0:b0 + blk.size + 1]
                out[p[0]:p[-1]] = comp.ranks(G1[blk], (p - p[0], pcol[p[0]:p[-1]]), exclude=lists(blk) if lists else None)[0]
            return out[back.reshape(-1)]
        return self._per_run(one, run)

    def complete_above(self, relation, threshold, rows=None, exclude=None, run=None, dtype='f64', block_rows=8192,
                       max_entries=2 ** 28):
        """``scipy.sparse.csr_matrix`` of shape ``(len(rows), n_j)``, float64, sorted indices: for each of ``rows``
        (default: every row object; otherwise an integer array in any order, duplicates allowed, results in that order)
        every column the model scores at or above ``threshold``, with its score -- what link prediction asks of
        ``complete(relation) >= threshold`` without forming it.  ``threshold`` is a scalar or one value per row; it is
        CAST TO THE SCORING TYPE of ``dtype`` ('f64' | 'f32' | 'bf16' -> f32) and the comparison ``score >= threshold``
        is made in that type, under IEEE rules: a NaN score or threshold selects nothing, ``-inf`` selects every
        admissible column.  ``exclude`` as for ``complete_topk`` (None, ``'known'`` or a scipy.sparse matrix of the
        relation's shape): an excluded pair is never returned.  The device counts, scans and fills ``block_rows`` rows at
        a time; nothing of size ``n_i x n_j`` is formed.  The size of the result depends on the data: once more than
        ``max_entries`` entries are found a ``DataFusionError`` is raised, before any array of that size is allocated.  A
        relation with a postprocessor is refused, as in ``complete_topk``.  ``n_run > 1`` and ``run=None``: a generator
        over the runs.  Extension of the reference API."""
        self._check_raw_scores(relation, 'complete_above')
        import scipy.sparse
        from .._engine import AboveLimit
        n_i, n_j = self._relation_shape(relation)
        rows = self._row_vector(rows, n_i)
        thr = np.asarray(threshold, dtype=np.float64)
        if thr.ndim > 1 or (thr.ndim == 1 and thr.shape != rows.shape):
            raise DataFusionError("threshold must be a scalar or one value per row (%d), not of shape %r"
                                  % (rows.size, tuple(thr.shape)))
        lists = self._exclusion_lists(relation, exclude, (n_i, n_j))
        step = max(1, int(block_rows))
        limit = int(max_entries)

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            indptr = np.zeros(rows.size + 1, dtype=np.int64)
            idx, val, found = [], [], 0
            for b0 in range(0, rows.size, step):
                blk = rows[b0:b0 + step]
                try:
                    p, i, v = comp.above(G1[blk], thr[b0:b0 + step] if thr.ndim else thr, exclude=lists(blk) if lists else None,
                                         max_entries=limit - found)
                except AboveLimit as over:
                    raise DataFusionError("complete_above: %d entries at or above the threshold in the first %d rows, "
                                          "max_entries = %d (raise the threshold or max_entries)"
                                          % (found + over.found, b0 + blk.size, limit))
                indptr[b0 + 1:b0 + blk.size + 1] = found + p[1:]
                found += int(p[-1])
                idx.append(i)
                val.append(v)
            out = scipy.sparse.csr_matrix((np.concatenate(val) if val else np.zeros(0), np.concatenate(idx) if idx else
                                           np.zeros(0, dtype=np.int32), indptr), shape=(rows.size, n_j))
            out.has_sorted_indices = True      # (ascending within a row by construction)
            return out
        return self._per_run(one, run)

    # ---- the n best pairs of a whole relation: a global selection on the device, never densified ---------------------------
    def _best_preamble(self, relation, method, n, rows, exclude, block_rows):
        self._check_raw_scores(relation, method)
        n = int(n)
        if n < 0:
            raise DataFusionError("%s: n = %d is negative" % (method, n))
        n_i, n_j = self._relation_shape(relation)
        rows = self._row_vector(rows, n_i)
        lists = self._exclusion_lists(relation, exclude, (n_i, n_j))
        step = max(1, int(block_rows))

        def blocks_of(G1):
            """A callable that returns a fresh iterator of (G_row_block, exclude) over the listed rows, in order."""
            def blocks():
                for b0 in range(0, rows.size, step):
                    blk = rows[b0:b0 + step]
                    yield G1[blk], lists(blk) if lists else None
            return blocks
        return n, rows, n_j, blocks_of

    def complete_kth(self, relation, n, rows=None, exclude=None, run=None, dtype='f64', block_rows=8192):
        """``(threshold, n_greater, n_equal)``: the ``n``-th largest score the model gives to any admissible pair of
        ``rows`` x all columns (``rows``: default every row object; a row listed twice is two rows) -- the cut-off to hand
        to ``complete_above`` for "the ``n`` most confident pairs", and the size to expect from it: ``n_greater`` pairs
        score above ``threshold`` and ``n_equal`` equal it, ``n_greater < n <= n_greater + n_equal``, and
        ``complete_above(relation, threshold, ...)`` with the same arguments returns exactly ``n_greater + n_equal``
        entries.  NaN scores and excluded pairs (``exclude`` as for ``complete_topk``) are no candidates.  With fewer than
        ``n`` candidates ``threshold`` is the smallest candidate score; with none, or ``n == 0``, it is NaN.  The device
        runs a radix select over the score tiles, ``block_rows`` rows at a time -- three passes in f32, six in f64 --
        and nothing of size ``n_i x n_j`` is formed; the result does not depend on ``block_rows``.  ``dtype`` and the
        refusal of post-processed relations as in ``complete_above``.  ``n_run > 1`` and ``run=None``: a generator over
        the runs.  Extension of the reference API."""
        n, rows, n_j, blocks_of = self._best_preamble(relation, 'complete_kth', n, rows, exclude, block_rows)

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            if n == 0 or rows.size == 0:
                return float('nan'), 0, 0
            return comp.kth(blocks_of(G1), n)[:3]
        return self._per_run(one, run)

    def complete_best(self, relation, n, rows=None, exclude=None, run=None, dtype='f64', block_rows=8192, ties='first',
                      max_entries=2 ** 28):
        """``scipy.sparse.csr_matrix`` of shape ``(len(rows), n_j)``, float64, sorted indices: the ``n`` best pairs of
        ``rows`` x all columns TOGETHER, with their scores -- link prediction's "the ``n`` most confident new pairs of this
        relation" without forming ``complete(relation)``.  Total order: higher score first, equal scores by lower position
        in ``rows``, then by lower column; a NaN score and an excluded pair (``exclude`` as for ``complete_topk``) are
        never selected.  ``ties='first'``: exactly ``min(n, candidates)`` entries, the first of that order;
        ``ties='all'``: every pair that equals the ``n``-th score as well, i.e. ``complete_above`` at
        ``complete_kth``'s threshold.  ``rows``: default every row object; otherwise an integer array in any order, a row
        listed twice is two rows.  ``n = 0`` gives an empty matrix; ``n > max_entries`` is refused before anything runs
        (and ``ties='all'`` once the ties push the result beyond it).  The device selects the threshold
        (``complete_kth``) and fills per block of ``block_rows`` rows; when the tie at the threshold holds more pairs than
        are wanted, two count passes per block say which rows the quota reaches, and only the row in which it runs out is
        trimmed on the host: nothing larger than the result is kept.  The bytes do not depend on ``block_rows``.
        ``dtype`` and the refusal of post-processed relations as in ``complete_above``.  ``n_run > 1`` and ``run=None``: a
        generator over the runs.  Extension of the reference API."""
        n, rows, n_j, blocks_of = self._best_preamble(relation, 'complete_best', n, rows, exclude, block_rows)
        import scipy.sparse
        from .._engine import AboveLimit
        if ties not in ('first', 'all'):
            raise DataFusionError("ties must be 'first' or 'all', not %r" % (ties,))
        limit = int(max_entries)
        if n > limit:
            raise DataFusionError("complete_best: n = %d, max_entries = %d" % (n, limit))

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            indptr = np.zeros(rows.size + 1, dtype=np.int64)
            idx, val = [np.zeros(0, dtype=np.int32)], [np.zeros(0)]
            T, greater, equal, cands = comp.kth(blocks_of(G1), n) if n and rows.size else (float('nan'), 0, 0, 0)
            if cands:
                want = greater + equal if ties == 'all' else min(n, cands)
                if want > limit:
                    raise DataFusionError("complete_best: %d entries with the ties at the %d-th score, max_entries = %d"
                                          % (want, n, limit))
                need = want - greater                   # of the `equal` pairs at T, the first `need` in (row, column) order
                ftype = np.dtype(comp.npd).type         # the next score above T in the SCORING type; above +inf: NaN, nothing
                strict = float(np.nextafter(ftype(T), ftype(np.inf))) if T < np.inf else np.nan
                plain = need == equal                   # the whole tie is wanted: above(T) as it is
                found, at = 0, 0
                for A, xl in blocks_of(G1)():
                    thr = T
                    cut = None
                    if not plain:
                        tied = np.diff(comp.above(A, T, exclude=xl, count_only=True)) - np.diff(comp.above(A, strict, exclude=xl, count_only=True))
                        before = np.cumsum(tied) - tied     # tied pairs of the block ahead of each row
                        thr = np.where(before < need, T, strict)
                        over = np.nonzero((before < need) & (before + tied > need))[0]
                        if over.size:                   # the row in which the quota runs out: its surplus goes, from the right
                            cut = (int(over[0]), int(before[over[0]] + tied[over[0]] - need))
                        need = max(0, need - int(tied.sum()))
                    try:
                        p, i, v = comp.above(A, thr, exclude=xl, max_entries=want - found + n_j)     # (+ the one row to trim)
                    except AboveLimit as over_limit:
                        raise RuntimeError("complete_best: %d entries in one block, the histograms said %d in all"
                                           % (over_limit.found, want))
                    if cut is not None:
                        q, surplus = cut
                        row = np.arange(p[q], p[q + 1])
                        drop = row[v[row] == T][-surplus:]
                        keep = np.ones(i.size, dtype=bool)
                        keep[drop] = False
                        i, v = i[keep], v[keep]
                        p = p.copy()
                        p[q + 1:] -= surplus
                    indptr[at + 1:at + A.shape[0] + 1] = found + p[1:]
                    found += int(p[-1])
                    at += A.shape[0]
                    idx.append(i)
                    val.append(v)
                if found != want:
                    raise RuntimeError("complete_best: %d entries filled, the histograms said %d (threshold %r, %d above, "
                                       "%d equal)" % (found, want, T, greater, equal))
            out = scipy.sparse.csr_matrix((np.concatenate(val), np.concatenate(idx), indptr), shape=(rows.size, n_j))
            out.has_sorted_indices = True      # (ascending within a row by construction)
            return out
        return self._per_run(one, run)

    # ---- the k best columns of every row for any k: one selection per row on the device, never densified -------------------
    def _row_preamble(self, relation, method, k, rows, exclude, block_rows):
        self._check_raw_scores(relation, method)
        n_i, n_j = self._relation_shape(relation)
        rows = self._row_vector(rows, n_i)
        want = np.asarray(k)
        if want.dtype.kind not in 'iu':
            raise DataFusionError("%s: k must be an integer or one integer per row, not %s" % (method, want.dtype))
        if want.ndim > 1 or (want.ndim == 1 and want.shape != rows.shape):
            raise DataFusionError("%s: k must be a scalar or one value per row (%d), not of shape %r"
                                  % (method, rows.size, tuple(want.shape)))
        if want.size and want.min() < 0:
            raise DataFusionError("%s: k = %d is negative" % (method, int(want.min())))
        scalar = want.ndim == 0
        want = np.ascontiguousarray(np.broadcast_to(want.astype(np.int64), rows.shape))
        lists = self._exclusion_lists(relation, exclude, (n_i, n_j))
        return rows, want, scalar, n_j, lists, max(1, int(block_rows))

    def complete_row_kth(self, relation, k, rows=None, exclude=None, run=None, dtype='f64', block_rows=8192):
        """``(thresholds float64 [n], n_greater int64 [n], n_equal int64 [n])``: for each of ``rows`` (default: every row
        object; otherwise an integer array in any order, a row listed twice is two rows) the ``k``-th largest score the model
        gives to an admissible column of that row -- ``k`` a non-negative integer or one per row, of ANY size: the per-row
        cut-off of Recall@100 / @1000, of R-precision (``k`` = a row's number of held-out pairs) and of candidate lists for a
        second stage --, the number of columns that score above it and the number that equal it.  NaN scores and excluded
        pairs (``exclude`` as for ``complete_topk``) are no candidates; with fewer than ``k`` candidates the threshold is
        the row's smallest candidate score; with none, or ``k == 0``, it is NaN and both counts are 0.
        ``complete_above(relation, thresholds, rows=rows, exclude=exclude)`` returns exactly ``n_greater + n_equal``
        entries per row.  The device runs one radix select per row over the score tiles, ``block_rows`` rows at a time --
        five passes in f32, ten in f64, no host round trip between them -- and nothing of size ``n_i x n_j`` is formed;
        the result does not depend on ``block_rows``.  ``dtype`` and the refusal of post-processed relations as in
        ``complete_above``.  ``n_run > 1`` and ``run=None``: a generator over the runs.  Extension of the reference API."""
        rows, want, _, n_j, lists, step = self._row_preamble(relation, 'complete_row_kth', k, rows, exclude, block_rows)

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            thr = np.empty(rows.size, dtype=np.float64)
            greater, equal = np.empty(rows.size, dtype=np.int64), np.empty(rows.size, dtype=np.int64)
            for b0 in range(0, rows.size, step):
                blk = rows[b0:b0 + step]
                thr[b0:b0 + step], greater[b0:b0 + step], equal[b0:b0 + step], _ = comp.row_kth(
                    G1[blk], want[b0:b0 + step], exclude=lists(blk) if lists else None)
            return thr, greater, equal
        return self._per_run(one, run)

    def complete_row_best(self, relation, k, rows=None, exclude=None, run=None, dtype='f64', block_rows=8192, ties='first',
                          ordered=False, max_entries=2 ** 28):
        """``scipy.sparse.csr_matrix`` of shape ``(len(rows), n_j)``, float64, sorted indices: for each of ``rows`` (default:
        every row object; otherwise an integer array in any order, a row listed twice is two rows) the ``k`` columns the
        model ranks highest, with their scores -- ``complete_topk`` without its limit of 64: ``k`` is a non-negative integer
        or one per row, of any size (``k_r = 0``: an empty row).  Order, candidates and ``exclude`` as for
        ``complete_topk``: higher score first, equal scores by lower column; NaN scores and excluded pairs never.
        ``ties='first'``: exactly ``min(k_r, candidates_r)`` entries per row, the first of that order -- of the pairs equal
        to the row's ``k_r``-th score the ones with the lowest columns; ``ties='all'``: every pair equal to the row's
        ``k_r``-th score as well, i.e. ``complete_above`` at ``complete_row_kth``'s thresholds.  ``ordered=True``
        (``ties='first'`` and a scalar ``k`` only): ``(indices int32 [n, k], scores float64 [n, k])`` in
        ``complete_topk``'s layout instead, best first, slots without a candidate ``-1`` / ``-inf``; for ``k <= 64`` these are
        ``complete_topk``'s arrays.  Per block of ``block_rows`` rows the device selects every row's threshold, counts and
        fills with the thresholds left where they are; the surplus of a tie is trimmed on the host, block by block, and
        nothing larger than one block's result is held beside the output.  ``sum(min(k_r, n_j)) > max_entries`` is refused
        before anything runs, and so is a block whose ties push the result beyond it.  The bytes do not depend on
        ``block_rows``.  ``dtype`` and the refusal of post-processed relations as in ``complete_above``.  ``n_run > 1`` and
        ``run=None``: a generator over the runs.  Extension of the reference API."""
        rows, want, scalar, n_j, lists, step = self._row_preamble(relation, 'complete_row_best', k, rows, exclude, block_rows)
        import scipy.sparse
        from .._engine import AboveLimit
        if ties not in ('first', 'all'):
            raise DataFusionError("ties must be 'first' or 'all', not %r" % (ties,))
        if ordered not in (False, True):
            raise DataFusionError("ordered must be True or False, not %r" % (ordered,))
        if ordered and (ties != 'first' or not scalar):
            raise DataFusionError("complete_row_best: ordered=True needs ties='first' and a scalar k")
        limit = int(max_entries)
        asked = int(np.minimum(want, n_j).sum())
        if asked > limit:
            raise DataFusionError("complete_row_best: %d entries asked for, max_entries = %d" % (asked, limit))
        width = int(np.asarray(k)) if scalar else 0

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            indptr = np.zeros(rows.size + 1, dtype=np.int64)
            idx, val, found = [np.zeros(0, dtype=np.int32)], [np.zeros(0)], 0
            for b0 in range(0, rows.size, step):
                blk = rows[b0:b0 + step]
                w = want[b0:b0 + step]
                try:
                    p, i, v, thr, greater, equal = comp.row_best(G1[blk], w, exclude=lists(blk) if lists else None,
                                                                 max_entries=limit - found)
                except AboveLimit as over:
                    raise DataFusionError("complete_row_best: %d entries with the ties in the first %d rows, max_entries = %d "
                                          "(lower k or raise max_entries)" % (found + over.found, b0 + blk.size, limit))
                if ties == 'first':
                    # of a row's pairs equal to its threshold the first min(k, greater + equal) - greater stay (columns ascend)
                    keep_eq = np.minimum(w, greater + equal) - greater
                    if (keep_eq < equal).any():
                        row_of = np.repeat(np.arange(blk.size), np.diff(p))
                        tied = v == thr[row_of]
                        before = np.concatenate([[0], np.cumsum(tied)])     # tied pairs of the block ahead of each entry
                        seen = before[1:] - before[p[:-1]][row_of]          # ... of the entry's own row, the entry included
                        keep = ~tied | (seen <= keep_eq[row_of])
                        i, v = i[keep], v[keep]
                        p = np.concatenate([[0], np.cumsum(np.bincount(row_of[keep], minlength=blk.size))]).astype(np.int64)
                indptr[b0 + 1:b0 + blk.size + 1] = found + p[1:]
                found += int(p[-1])
                idx.append(i)
                val.append(v)
            idx, val = np.concatenate(idx), np.concatenate(val)
            if ordered:
                oi = np.full((rows.size, width), -1, dtype=np.int32)
                ov = np.full((rows.size, width), -np.inf)
                row_of = np.repeat(np.arange(rows.size), np.diff(indptr))
                o = np.lexsort((idx, -val, row_of))                     # by row, then value descending, then column ascending
                slot = np.arange(idx.size) - indptr[row_of]             # (row_of[o] == row_of: the rows stay in place)
                oi[row_of, slot] = idx[o]
                ov[row_of, slot] = val[o]
                return oi, ov
            out = scipy.sparse.csr_matrix((val, idx, indptr), shape=(rows.size, n_j))
            out.has_sorted_indices = True      # (ascending within a row by construction)
            return out
        return self._per_run(one, run)


# ---- persistence of a fitted model (the reference has none: its accessors base.py:35-56,
# 169-189 are the only consumers of factors_ / backbones_) ----------------------------------------------
_FORMAT = 'skfusion_amd.fit/1'


def _plain(value):
    """Constructor parameters that survive JSON; callables, RandomState objects ... are dropped (None)."""
    if value is None or isinstance(value, (bool, int, float, str)):
        return value
    if isinstance(value, (np.integer, np.floating)):
        return value.item()
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    return None


def save_fit(fuser, path):
    """Fitted Dfmf / Dfmc -> ONE ``.npz`` file: every factor G (per object type and run) and backbone S (per
    relation and run) as float64 arrays ``G/<type index>/<run>``, ``S/<relation index>/<run>``, plus a JSON
    header (format tag, class, constructor parameters, object types with rank and size, relations by row / column
    type and position among the relations of that pair)."""
    import json
    graph = fuser.fusion_graph
    types = list(graph.object_types)
    rels = list(graph.relations)
    n_run = int(fuser.n_run)
    arrays = {}
    for a, ot in enumerate(types):
        runs = fuser.factors_[ot]
        if len(runs) != n_run:
            raise DataFusionError("Object type %s has %d fitted factors, expected %d" % (ot.name, len(runs), n_run))
        for k, G in enumerate(runs):
            arrays['G/%d/%d' % (a, k)] = np.asarray(G, dtype=np.float64)
    seen = {}
    rel_meta = []
    for b, rel in enumerate(rels):
        pair = (rel.row_type.name, rel.col_type.name)
        pos = seen.get(pair, 0)
        seen[pair] = pos + 1
        rel_meta.append({'row': pair[0], 'col': pair[1], 'name': str(getattr(rel, 'name', '') or ''), 'position': pos,
                         'shape': [int(d) for d in np.shape(rel.data)]})
        # a same-type relation is a constraint (Theta): it has no backbone.  `.get`: no entry is inserted into the
        # defaultdict, so `backbone(theta_relation)` keeps raising "Unknown relation." after a save
        runs = fuser.backbones_.get(rel, [])
        rel_meta[-1]['n_backbones'] = len(runs)
        for k, S in enumerate(runs):
            arrays['S/%d/%d' % (b, k)] = np.asarray(S, dtype=np.float64)
    meta = {'format': _FORMAT, 'class': type(fuser).__name__, 'n_run': n_run,
            'params': {k: _plain(v) for k, v in (fuser._params or {}).items()},
            'object_types': [{'name': str(ot.name), 'rank': int(ot.rank),
                              'n_objects': int(np.shape(fuser.factors_[ot][0])[0])} for ot in types],
            'relations': rel_meta}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode('utf-8'), dtype=np.uint8)
    with open(path, 'wb') as fh:
        np.savez_compressed(fh, **arrays)
    return path


def load_fit(path, fusion_graph=None):
    """Inverse of ``save_fit``: a fuser of the saved class whose ``factor`` / ``backbone`` / ``complete`` /
    ``chain`` accessors work (including the generator convention for ``n_run > 1``).  With ``fusion_graph`` the
    factors are attached to ITS object types / relations (matched by name and by position among the relations of
    a type pair; sizes are checked); without one a skeleton graph of the saved types and relation shapes is
    built (relation data: read-only NaN views that take no memory)."""
    import json
    from .fusion_graph import FusionGraph, ObjectType, Relation
    with np.load(path, allow_pickle=False) as z:
        meta = json.loads(bytes(z['meta'].tobytes()).decode('utf-8'))
        if meta.get('format') != _FORMAT:
            raise DataFusionError("Not a saved fusion model: %r" % (meta.get('format'),))
        arrays = {k: z[k] for k in z.files if k != 'meta'}
    if fusion_graph is None:
        by_name = {t['name']: ObjectType(t['name'], t['rank']) for t in meta['object_types']}
        fusion_graph = FusionGraph([Relation(np.broadcast_to(np.nan, tuple(r['shape'])), by_name[r['row']],
                                             by_name[r['col']], name=r['name']) for r in meta['relations']])
    from . import decomposition
    cls = getattr(decomposition, meta['class'], None)
    if cls is None or not issubclass(cls, FusionFit):
        raise DataFusionError("Unknown fuser class %r" % (meta['class'],))
    params = {k: v for k, v in meta['params'].items() if v is not None}
    fuser = cls(**params)
    fuser.fusion_graph = fusion_graph
    n_run = int(meta['n_run'])
    names = {ot.name: ot for ot in fusion_graph.object_types}
    for a, t in enumerate(meta['object_types']):
        if t['name'] not in names:
            raise DataFusionError("Object type %s is not included in the fusion scheme" % t['name'])
        ot = names[t['name']]
        for k in range(n_run):
            G = arrays['G/%d/%d' % (a, k)]
            if G.shape != (t['n_objects'], t['rank']):
                raise DataFusionError("Factor of %s has shape %r" % (t['name'], G.shape))
            fuser.factors_[ot].append(G)
    for b, r in enumerate(meta['relations']):
        cands = list(fusion_graph.get_relations(names[r['row']], names[r['col']]))
        if r['position'] >= len(cands):
            raise DataFusionError("Relation %s -> %s #%d is not in the fusion graph" % (r['row'], r['col'], r['position']))
        rel = cands[r['position']]
        if list(np.shape(rel.data)) != list(r['shape']):
            raise DataFusionError("Relation %s -> %s: data shape %r, saved %r"
                                  % (r['row'], r['col'], np.shape(rel.data), r['shape']))
        have = int(r.get('n_backbones', 0 if r['row'] == r['col'] else n_run))
        for k in range(have):              # (constraints were saved without backbones)
            fuser.backbones_[rel].append(arrays['S/%d/%d' % (b, k)])
    return fuser


class FusionTransform(FusionBase):
    """Base of the online (fold-in) transformers: attributes ``target``, ``fusion_graph``,
    ``fuser``."""

    def _validate_graph(self):
        if self.target not in self.fusion_graph.object_types:
            raise DataFusionError("Object type %s is not included in the fusion scheme."
                                  % self.target.name)
        for relation in self.fusion_graph.relations:
            if self.target not in (relation.row_type, relation.col_type):
                raise DataFusionError("Relation must include target object type: %s."
                                      % self.target.name)

    def _chain_source(self, row_type, run):
        # the paths, backbones and column factors are the fitted model's; the rows are the target's NEW objects
        # (reference examples: profile(fuser, transformer) takes transformer.factor(gene) with fuser.chain / backbone)
        if row_type is not None and row_type is not self.target:
            raise DataFusionError("Starting type should be target type: %s" % self.target.name)
        return self.fuser, self.factor(self.target, run)

    def chain(self, row_type=None, col_type=None):
        if row_type is not None and col_type is not None and row_type is not self.target:
            raise DataFusionError("Starting type should be target type: %s" % self.target.name)
        if col_type is None:
            col_type = row_type
        return FusionBase.chain(self, self.target, col_type)
