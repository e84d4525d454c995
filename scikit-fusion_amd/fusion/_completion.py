"""The completion operators of a fitted model (``FusionFit`` inherits them): predictions at given pairs, the k best columns of
a row, ranks of held-out pairs, scores above a threshold, the n best pairs of a relation, the k best columns of every row
for any k and the histogram of a relation's scores with the ROC / PR curves read from it -- all on the device, never
densified (``_complete.DeviceCompleter``).

Every operator is written from the same pieces: one ``_Query`` (the checked rows, the relation's shape, the exclusion lists
and the walk over row blocks), for the CSR-returning ones one ``_CsrRows`` (the result, filled block by block, and the
translation of the device's ``AboveLimit``), and ``_per_run`` for the runs.
"""
import collections
import contextlib

import numpy as np

from .._complete import AboveLimit, DeviceCompleter
from .._native import SKF_TOPK_MAX
from .base import DataFusionError


class _Query(object):
    """What an operator asks of ``relation``: the rows (``rows=None``: every row object), the relation's shape, the
    exclusion lists and the block size, checked once for all runs (``method``: the operator's own name, for its refusals)."""

    def __init__(self, fit, relation, method, rows, exclude, block_rows):
        fit._check_raw_scores(relation, method)
        self.n_i, self.n_j = fit._relation_shape(relation)
        self.rows = fit._row_vector(rows, self.n_i)
        self.lists = fit._exclusion_lists(relation, exclude, (self.n_i, self.n_j))
        self.step = max(1, int(block_rows))

    def blocks(self, rows=None):
        """``(b0, blk, exclude)`` for every block of at most ``step`` of the rows (default: the query's own), in order: its
        offset, its row indices and its exclusion lists as ``DeviceCompleter`` takes them (None without lists)."""
        rows = self.rows if rows is None else rows
        for b0 in range(0, rows.size, self.step):
            blk = rows[b0:b0 + self.step]
            yield b0, blk, self.lists(blk) if self.lists else None

    def blocks_of(self, G1):
        """A callable that returns a fresh iterator of (G_row_block, exclude) over the rows, in order: what
        ``DeviceCompleter.kth`` walks once per pass."""
        return lambda: ((G1[blk], xl) for _, blk, xl in self.blocks())


class _CsrRows(object):
    """The ``csr_matrix`` an operator returns, filled block by block: ``indices`` int32, ``data`` float64, ``indptr`` int64,
    also when nothing was added.  ``limit``: the operator's ``max_entries``."""

    def __init__(self, n_rows, limit=None):
        self.indptr = np.zeros(n_rows + 1, dtype=np.int64)
        self.idx, self.val = [np.zeros(0, dtype=np.int32)], [np.zeros(0)]
        self.found = self.at = 0               # entries and rows added so far
        self.limit = limit

    @contextlib.contextmanager
    def room(self, n_rows, message):
        """Yields the entries the next block of ``n_rows`` rows may hold; an ``AboveLimit`` of the device inside becomes the
        operator's ``DataFusionError``: ``message % (entries found, rows walked, max_entries)``."""
        try:
            yield self.limit - self.found
        except AboveLimit as over:
            raise DataFusionError(message % (self.found + over.found, self.at + n_rows, self.limit))

    def add(self, n_rows, p, i, v):
        """The next ``n_rows`` rows: their CSR ``(p, i, v)`` as the device returns a block's."""
        self.indptr[self.at + 1:self.at + n_rows + 1] = self.found + p[1:]
        self.found += int(p[-1])
        self.at += n_rows
        self.idx.append(i)
        self.val.append(v)

    def entries(self):
        return np.concatenate(self.idx), np.concatenate(self.val)

    def finish(self, n_j):
        import scipy.sparse
        idx, val = self.entries()
        out = scipy.sparse.csr_matrix((val, idx, self.indptr), shape=(self.indptr.size - 1, n_j))
        out.has_sorted_indices = True      # (ascending within a row by construction)
        return out


def _per_row(value, n_rows, what, dtype=None):
    """``value`` -- a scalar or one value per row -- as an array of no or one dimension."""
    value = np.asarray(value, dtype=dtype)
    if value.ndim > 1 or (value.ndim == 1 and value.shape != (n_rows,)):
        raise DataFusionError("%s must be a scalar or one value per row (%d), not of shape %r"
                              % (what, n_rows, tuple(value.shape)))
    return value


def _row_wants(method, k, n_rows):
    """``(want int64 [n_rows], k was a scalar)`` for ``k``, a non-negative integer or one per row."""
    want = np.asarray(k)
    if want.dtype.kind not in 'iu':
        raise DataFusionError("%s: k must be an integer or one integer per row, not %s" % (method, want.dtype))
    want = _per_row(want, n_rows, '%s: k' % method)
    if want.size and want.min() < 0:
        raise DataFusionError("%s: k = %d is negative" % (method, int(want.min())))
    return np.ascontiguousarray(np.broadcast_to(want.astype(np.int64), (n_rows,))), want.ndim == 0


def _check_ties(ties):
    if ties not in ('first', 'all'):
        raise DataFusionError("ties must be 'first' or 'all', not %r" % (ties,))


class CompletionOperators(object):
    """Mixin of ``FusionFit``: works from ``factor``, ``backbone``, ``fusion_graph`` and ``n_run`` alone, and never calls
    ``complete`` / ``_reconstruct``."""

    # ---- predictions at given pairs and the k best columns of a row, on the device, never densified ----------------------
    # The reference answers both from the dense product (base.py:119-146; examples/movielens_completion.py:121-126 reads
    # R12_pred[hidden]); here nothing of size n_i x n_j is formed on the host or in HBM (`_complete.DeviceCompleter`).
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
        return self._pair_lists(exclude, shape, 'exclude')

    @staticmethod
    def _pair_lists(pairs, shape, what):
        """A function ``rows -> (indptr int64, indices int32)`` for the stored entries of the scipy.sparse matrix ``pairs`` of
        the relation's ``shape``: CSR with strictly ascending columns, sliced per block, never expanded."""
        import scipy.sparse
        if tuple(pairs.shape) != tuple(shape):
            raise DataFusionError("%s has shape %r, the relation %r" % (what, tuple(pairs.shape), tuple(shape)))
        csr = scipy.sparse.csr_matrix(pairs)        # (duplicates of a COO matrix are summed; stored zeros stay entries)
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
        q = _Query(self, relation, 'complete_topk', rows, exclude, block_rows)
        k = int(k)
        if not 1 <= k <= SKF_TOPK_MAX:
            raise DataFusionError("k = %d outside 1 .. %d" % (k, SKF_TOPK_MAX))

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            idx = np.empty((q.rows.size, k), dtype=np.int32)
            val = np.empty((q.rows.size, k), dtype=np.float64)
            for b0, blk, xl in q.blocks():
                idx[b0:b0 + blk.size], val[b0:b0 + blk.size] = comp.topk(G1[blk], k, exclude=xl)
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
        q = _Query(self, relation, 'complete_ranks', None, exclude, block_rows)      # (its own rows are not used: see below)
        rows, cols, n_i, n_j = self._pair_vectors(relation, rows, cols)
        # the distinct pairs in (row, column) order are the target CSR over the distinct rows; `back` leads home
        key, back = np.unique(rows.astype(np.int64) * n_j + cols.astype(np.int64), return_inverse=True)
        prow, pcol = key // max(n_j, 1), (key % max(n_j, 1)).astype(np.int32)
        urows, first = np.unique(prow, return_index=True)
        ptr = np.append(first, key.size).astype(np.int64)

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            out = np.empty(key.size, dtype=np.int64)
            for b0, blk, xl in q.blocks(urows):              # (the walk is over the DISTINCT rows of the pairs)
                p = ptr[b0:b0 + blk.size + 1]
                out[p[0]:p[-1]] = comp.ranks(G1[blk], (p - p[0], pcol[p[0]:p[-1]]), exclude=xl)[0]
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
        q = _Query(self, relation, 'complete_above', rows, exclude, block_rows)
        thr = _per_row(threshold, q.rows.size, 'threshold', dtype=np.float64)
        limit = int(max_entries)

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            out = _CsrRows(q.rows.size, limit)
            for b0, blk, xl in q.blocks():
                with out.room(blk.size, "complete_above: %d entries at or above the threshold in the first %d rows, "
                                        "max_entries = %d (raise the threshold or max_entries)") as room:
                    csr = comp.above(G1[blk], thr[b0:b0 + blk.size] if thr.ndim else thr, exclude=xl, max_entries=room)
                out.add(blk.size, *csr)
            return out.finish(q.n_j)
        return self._per_run(one, run)

    # ---- the n best pairs of a whole relation: a global selection on the device, never densified ---------------------------
    def _best_query(self, relation, method, n, rows, exclude, block_rows):
        q = _Query(self, relation, method, rows, exclude, block_rows)
        n = int(n)
        if n < 0:
            raise DataFusionError("%s: n = %d is negative" % (method, n))
        return q, n

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
        q, n = self._best_query(relation, 'complete_kth', n, rows, exclude, block_rows)

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            if n == 0 or q.rows.size == 0:
                return float('nan'), 0, 0
            return comp.kth(q.blocks_of(G1), n)[:3]
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
        q, n = self._best_query(relation, 'complete_best', n, rows, exclude, block_rows)
        _check_ties(ties)
        limit = int(max_entries)
        if n > limit:
            raise DataFusionError("complete_best: n = %d, max_entries = %d" % (n, limit))

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            out = _CsrRows(q.rows.size)
            T, greater, equal, cands = comp.kth(q.blocks_of(G1), n) if n and q.rows.size else (float('nan'), 0, 0, 0)
            if cands:
                want = greater + equal if ties == 'all' else min(n, cands)
                if want > limit:
                    raise DataFusionError("complete_best: %d entries with the ties at the %d-th score, max_entries = %d"
                                          % (want, n, limit))
                need = want - greater                   # of the `equal` pairs at T, the first `need` in (row, column) order
                ftype = np.dtype(comp.npd).type         # the next score above T in the SCORING type; above +inf: NaN, nothing
                strict = float(np.nextafter(ftype(T), ftype(np.inf))) if T < np.inf else np.nan
                plain = need == equal                   # the whole tie is wanted: above(T) as it is
                for _, blk, xl in q.blocks():
                    A = G1[blk]
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
                        p, i, v = comp.above(A, thr, exclude=xl, max_entries=want - out.found + q.n_j)     # (+ the one row to trim)
                    except AboveLimit as over_limit:
                        raise RuntimeError("complete_best: %d entries in one block, the histograms said %d in all"
                                           % (over_limit.found, want))
                    if cut is not None:
                        row, surplus = cut
                        of_row = np.arange(p[row], p[row + 1])
                        drop = of_row[v[of_row] == T][-surplus:]
                        keep = np.ones(i.size, dtype=bool)
                        keep[drop] = False
                        i, v = i[keep], v[keep]
                        p = p.copy()
                        p[row + 1:] -= surplus
                    out.add(blk.size, p, i, v)
                if out.found != want:
                    raise RuntimeError("complete_best: %d entries filled, the histograms said %d (threshold %r, %d above, "
                                       "%d equal)" % (out.found, want, T, greater, equal))
            return out.finish(q.n_j)
        return self._per_run(one, run)

    # ---- the k best columns of every row for any k: one selection per row on the device, never densified -------------------
    def _row_query(self, relation, method, k, rows, exclude, block_rows):
        q = _Query(self, relation, method, rows, exclude, block_rows)
        return (q,) + _row_wants(method, k, q.rows.size)

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
        q, want, _ = self._row_query(relation, 'complete_row_kth', k, rows, exclude, block_rows)

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            thr = np.empty(q.rows.size, dtype=np.float64)
            greater, equal = np.empty(q.rows.size, dtype=np.int64), np.empty(q.rows.size, dtype=np.int64)
            for b0, blk, xl in q.blocks():
                b1 = b0 + blk.size
                thr[b0:b1], greater[b0:b1], equal[b0:b1], _ = comp.row_kth(G1[blk], want[b0:b1], exclude=xl)
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
        q, want, scalar = self._row_query(relation, 'complete_row_best', k, rows, exclude, block_rows)
        _check_ties(ties)
        if ordered not in (False, True):
            raise DataFusionError("ordered must be True or False, not %r" % (ordered,))
        if ordered and (ties != 'first' or not scalar):
            raise DataFusionError("complete_row_best: ordered=True needs ties='first' and a scalar k")
        limit = int(max_entries)
        asked = int(np.minimum(want, q.n_j).sum())
        if asked > limit:
            raise DataFusionError("complete_row_best: %d entries asked for, max_entries = %d" % (asked, limit))
        width = int(np.asarray(k)) if scalar else 0

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            out = _CsrRows(q.rows.size, limit)
            for b0, blk, xl in q.blocks():
                w = want[b0:b0 + blk.size]
                with out.room(blk.size, "complete_row_best: %d entries with the ties in the first %d rows, max_entries = %d "
                                        "(lower k or raise max_entries)") as room:
                    p, i, v, thr, greater, equal = comp.row_best(G1[blk], w, exclude=xl, max_entries=room)
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
                out.add(blk.size, p, i, v)
            if ordered:
                idx, val = out.entries()
                oi = np.full((q.rows.size, width), -1, dtype=np.int32)
                ov = np.full((q.rows.size, width), -np.inf)
                row_of = np.repeat(np.arange(q.rows.size), np.diff(out.indptr))
                o = np.lexsort((idx, -val, row_of))                     # by row, then value descending, then column ascending
                slot = np.arange(idx.size) - out.indptr[row_of]         # (row_of[o] == row_of: the rows stay in place)
                oi[row_of, slot] = idx[o]
                ov[row_of, slot] = val[o]
                return oi, ov
            return out.finish(q.n_j)
        return self._per_run(one, run)

    # ---- how the scores of a relation are distributed: histograms and ROC / PR curves on the device, never densified -------
    def _hist_query(self, relation, method, edges, rows, exclude, targets, what, block_rows):
        """``(q, edges float64 [n], lists of the target pairs or None)`` of the two operators below, checked."""
        import scipy.sparse
        q = _Query(self, relation, method, rows, exclude, block_rows)
        tl = None
        if targets is not None:
            if not scipy.sparse.issparse(targets):
                raise DataFusionError("%s must be a scipy.sparse matrix, not %s" % (what, type(targets).__name__))
            tl = self._pair_lists(targets, (q.n_i, q.n_j), what)
        if edges is not None:
            edges = np.asarray(edges)
            if edges.dtype.kind not in 'fiu' or edges.ndim != 1 or edges.size < 1:
                raise DataFusionError("%s: edges must be a one-dimensional array of at least one number, not %s of shape %r"
                                      % (method, edges.dtype, tuple(edges.shape)))
            edges = edges.astype(np.float64)
            if np.isnan(edges).any() or (edges[1:] < edges[:-1]).any():
                raise DataFusionError("%s: edges must not hold NaN and must not descend" % method)
        return q, edges, tl

    @staticmethod
    def _hist_blocks(q, G1, tl):
        """What ``DeviceCompleter.histogram`` walks once per chunk of edges."""
        return lambda: ((G1[blk], xl, tl(blk) if tl else None) for _, blk, xl in q.blocks())

    def complete_histogram(self, relation, edges, rows=None, exclude=None, targets=None, run=None, dtype='f64', block_rows=8192):
        """``counts int64 [len(edges) + 1]``: how the scores the model gives to the admissible pairs of ``rows`` x all columns
        (``rows``: default every row object; a row listed twice is two rows) are distributed over the bins that ``edges`` cut:
        ``counts[b]`` pairs score in bin ``b = #{t : edges[t] <= score}``, so that ``counts[t + 1:].sum()`` pairs score at or
        above ``edges[t]`` -- the size ``complete_above`` returns at that threshold, for every threshold at once and in one
        walk over the score tiles.  ``edges`` is one-dimensional, of any length, without NaN and non-decreasing (``-inf`` and
        ``+inf`` are ordinary edges); it is CAST TO THE SCORING TYPE of ``dtype`` ('f64' | 'f32' | 'bf16' -> f32), as
        ``threshold`` is in ``complete_above``, and the comparison is made in that type: a cast that merges two edges leaves
        an empty bin.  NaN scores and excluded pairs (``exclude`` as for ``complete_topk``) are counted nowhere.  ``targets``
        -- a scipy.sparse matrix of the relation's shape whose stored entries are pairs of interest, e.g. a gold standard;
        kept as CSR, sliced per block, never expanded -- gives ``(counts, target_counts)``: ``target_counts[b]`` of the
        ``counts[b]`` pairs are targets (a target that is excluded or scores NaN is counted in neither).  The device bins
        ``block_rows`` rows at a time, 2047 edges per walk; nothing of size ``n_i x n_j`` is formed and the result does not
        depend on ``block_rows``.  A relation with a postprocessor is refused, as in ``complete_topk``.  ``n_run > 1`` and
        ``run=None``: a generator over the runs.  Extension of the reference API."""
        q, edges, tl = self._hist_query(relation, 'complete_histogram', edges, rows, exclude, targets, 'targets', block_rows)
        if edges is None:
            raise DataFusionError("complete_histogram: edges must be a one-dimensional array of at least one number, not None")

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            counts, target_counts, _ = comp.histogram(self._hist_blocks(q, G1, tl), edges)
            if tl and target_counts is None:            # (no row at all)
                target_counts = np.zeros_like(counts)
            return (counts, target_counts) if tl else counts
        return self._per_run(one, run)

    def complete_curve(self, relation, positives, edges=None, n_edges=2047, rows=None, exclude=None, run=None, dtype='f64',
                       block_rows=8192):
        """The global (micro-averaged) ROC and precision-recall curves of the model's scores against the gold standard
        ``positives`` -- a scipy.sparse matrix of the relation's shape whose stored entries are the positive pairs -- over the
        admissible pairs of ``rows`` x all columns, without the dense product the reference's users hand to ``roc_auc_score``
        (examples/pharma_chaining.py:100).  Returns a ``CompletionCurve``:
          ``thresholds`` float64, ascending (``edges`` in the scoring type); ``predicted[t]`` the candidates -- admissible pairs
          whose score is not NaN -- scoring at or above ``thresholds[t]``; ``true_positives[t]`` the positives among them;
          ``n_candidates``; ``n_positives`` the positives that are candidates (an excluded or NaN-scored positive is not
          counted) and ``n_positives_given`` the stored entries of ``positives`` in ``rows``; ``precision``, ``recall`` and
          ``fpr`` float64 per threshold, NaN where the denominator is 0; ``auroc = (lo, hi)``, the exact bounds of the area
          under the ROC curve given the histogram: within a bin every negative ahead of every positive, and the reverse --
          ``hi - lo`` is the share of (positive, negative) pairs that meet in one bin; when every bin holds one distinct score
          ``(lo + hi) / 2`` is the mid-rank AUROC exactly.  ``(nan, nan)`` without a positive or without a negative.
        ``edges=None`` takes the distinct values of up to ``n_edges`` evenly spaced order statistics of the positives' own
        scores (``complete_entries``, cast to the scoring type): that puts the resolution where the curve moves, and the width
        ``hi - lo`` the result carries is all that is promised of it.  ``edges``, ``exclude``, ``dtype``, ``block_rows`` and the
        refusal of post-processed relations as in ``complete_histogram``.  ``n_run > 1`` and ``run=None``: a generator over the
        runs.  Extension of the reference API."""
        q, edges, tl = self._hist_query(relation, 'complete_curve', edges, rows, exclude, positives, 'positives', block_rows)
        if tl is None:
            raise DataFusionError("positives must be a scipy.sparse matrix, not None")
        n_edges = int(n_edges)
        if n_edges < 1:
            raise DataFusionError("complete_curve: n_edges = %d, at least 1 is needed" % n_edges)
        given = [tl(blk) for _, blk, _ in q.blocks()]
        n_given = int(sum(p[-1] for p, _ in given))

        def one(r):
            G1, comp = self._completer(relation, r, dtype)
            e = edges
            if e is None:
                prow = np.concatenate([np.repeat(blk, np.diff(p)) for (_, blk, _), (p, _) in zip(q.blocks(), given)] + [np.zeros(0, dtype=np.int64)])
                pcol = np.concatenate([i for _, i in given] + [np.zeros(0, dtype=np.int32)])
                s = comp.entries(G1, prow, pcol).astype(comp.npd)
                s = np.sort(s[~np.isnan(s)])
                e = np.unique(s[np.unique(np.linspace(0, s.size - 1, min(n_edges, s.size)).round().astype(np.int64))]) if s.size else np.zeros(1)
            e = np.asarray(e, dtype=np.float64).astype(comp.npd).astype(np.float64)
            counts, pos, _ = comp.histogram(self._hist_blocks(q, G1, tl), e)
            if pos is None:                             # (no row at all)
                pos = np.zeros_like(counts)
            return curve_of(e, counts, pos, n_given)
        return self._per_run(one, run)


CompletionCurve = collections.namedtuple('CompletionCurve', 'thresholds predicted true_positives n_candidates n_positives '
                                         'n_positives_given precision recall fpr auroc')


def auroc_bounds(counts, target_counts):
    """``(lo, hi)`` as ``fractions.Fraction``, or None without a positive or without a negative: the area under the ROC curve
    of a histogram with ``target_counts[b]`` positives among the ``counts[b]`` scores of bin ``b`` (bins ascending), with every
    negative of a bin ahead of every positive of it, and the reverse.  Python integers throughout."""
    import fractions
    pos = [int(v) for v in target_counts]
    neg = [int(c) - p for c, p in zip(counts, pos)]
    P, N = sum(pos), sum(neg)
    if P == 0 or N == 0:
        return None
    below = lo = tie = 0
    for p, n in zip(pos, neg):
        lo += p * below
        tie += p * n
        below += n
    return fractions.Fraction(lo, P * N), fractions.Fraction(lo + tie, P * N)


def curve_of(thresholds, counts, target_counts, n_positives_given):
    """The ``CompletionCurve`` of one histogram (``counts`` / ``target_counts`` int64 [len(thresholds) + 1])."""
    predicted = np.cumsum(counts[::-1])[::-1][1:].astype(np.int64)
    tp = np.cumsum(target_counts[::-1])[::-1][1:].astype(np.int64)
    cands, P = int(counts.sum()), int(target_counts.sum())
    N = cands - P
    nan = np.full(predicted.size, np.nan)
    precision = np.divide(tp, predicted, out=nan.copy(), where=predicted > 0)
    recall = tp / float(P) if P else nan.copy()
    fpr = (predicted - tp) / float(N) if N else nan.copy()
    bounds = auroc_bounds(counts, target_counts)
    auroc = (float('nan'), float('nan')) if bounds is None else (float(bounds[0]), float(bounds[1]))
    return CompletionCurve(np.asarray(thresholds, dtype=np.float64), predicted, tp, cands, P, int(n_positives_given), precision, recall,
                           fpr, auroc)
