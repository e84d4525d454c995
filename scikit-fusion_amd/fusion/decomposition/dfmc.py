"""``Dfmc`` -- data fusion by matrix completion, class layer of the drop-in boundary
(reference ``skfusion/fusion/decomposition/dfmc.py:18-115``).  Masked entries of a relation
(numpy masked arrays that are still masked after fill + preprocess) are treated as unknown
and completed by the model; the relation objects' data is never modified."""
import numpy as np

from . import _dfmc
from .dfmf import _Fuser, DfmfTransform

__all__ = ['Dfmc', 'DfmcTransform']


class Dfmc(_Fuser):
    """Parameters identical to the reference: max_iter=100, init_type='random_c', n_run=1,
    stopping=None, stopping_system=None, verbose=0, compute_err=False, callback=None,
    random_state=None, n_jobs=1.  Addition: dtype='f64' | 'f32'.  A relation given as its known entries
    (``Relation(scipy.sparse matrix, ..., unstored='unknown')``) is fitted on those entries alone with shard='runs'
    (see ``Relation``) and with shard='owned', where every rank uploads the known entries of its owned rows only (the
    whole matrix stays on every process's host for the initialisers; 'rows' / 'relations' expand it); such a relation with
    fill_value 'row_mean' / 'col_mean' (no mask is left) as entries plus rank one with shard='runs' (``sparse_relations``,
    ``filled_entries_apply``); one whose unstored entries are zero on its stored entries (``sparse_relations``, see ``Dfmf``); a
    ``scipy.sparse`` constraint as its entries (``sparse_constraints``, see ``Dfmf``).
    validation, patience, min_delta, check_every, restore_best: held-out pairs scored inside the fit, early stopping on their
    pooled squared error and the best iterate returned, as in ``Dfmf`` -- the held-out pairs of a relation with missing
    values must be among its UNKNOWN cells (``heldout_lists`` refuses a pair the training relation knows)."""

    _variant = 'dfmc'
    _keeps_masks = True
    _takes_known_entries = True
    _shares_launches = False    # (the restarts of a Dfmc fit have no shared-launch branch)

    def __init__(self, max_iter=100, init_type='random_c', n_run=1, stopping=None,
                 stopping_system=None, verbose=0, compute_err=False, callback=None,
                 random_state=None, n_jobs=1, dtype='f64', shard='runs', device_fill=False, sparse_relations=None,
                 sparse_constraints=None, init_device=None, validation=None, patience=None, min_delta=0.0, check_every=8,
                 restore_best=True):
        super(Dfmc, self).__init__()
        self._set_params(vars())

    def _solve(self, M, **kw):
        return _dfmc.dfmc(M=M, **kw)


def unknown_cells(relation):
    """Whether a relation between two object types holds cells that a completion model leaves to the model: a
    ``scipy.sparse`` matrix given with ``unstored='unknown'`` (whatever its density), or a ``MaskedArray`` that masks at
    least one cell."""
    if relation.row_type == relation.col_type:
        return False
    return relation.is_known_entries() or bool(np.ma.is_masked(relation.data))


def known_lists(relation, by_col, fill):
    """The KNOWN cells of `relation` (``unknown_cells``) as ``_engine.KnownEntries(unstored='unknown')``, compressed along its
    rows or, `by_col`, its columns; never a dense step for a scipy.sparse matrix.  Duplicates are summed, indices sorted,
    stored zeros kept; a stored (or unmasked) value that is not finite is unknown, like a cell that is not stored.  `fill`
    is what the container carries for the unknown cells: the initialisers read it, nothing else does."""
    from ..._engine import KnownEntries
    import scipy.sparse
    shape = tuple(relation.data.shape)
    if relation.is_known_entries():
        m = (scipy.sparse.csc_matrix if by_col else scipy.sparse.csr_matrix)(relation.data, dtype=np.float64, copy=True)
        m.sum_duplicates()
        m.sort_indices()
        indptr, indices, values = m.indptr, m.indices, m.data
    else:
        # the unmasked cells of a MaskedArray, walked along the compressed side (row-major over the view whose rows it is)
        view = relation.data.T if by_col else relation.data
        known = ~np.ma.getmaskarray(view)
        outer, indices = np.nonzero(known)
        values = np.asarray(np.ma.getdata(view), dtype=np.float64)[outer, indices]
        indptr = np.zeros(view.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(outer, minlength=view.shape[0]), out=indptr[1:])
    finite = np.isfinite(values)
    if not finite.all():
        outer = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))[finite]
        indices, values = indices[finite], values[finite]
        indptr = np.zeros(indptr.size, dtype=np.int64)
        np.cumsum(np.bincount(outer, minlength=indptr.size - 1), out=indptr[1:])
    return KnownEntries(indptr, indices, values, shape, fill=fill, by_col=by_col)


class DfmcTransform(DfmfTransform):
    """Online transformer of new objects into a fitted completion model, on their KNOWN entries alone.

    ``DfmfTransform`` (the reference's fold-in) has no notion of an unknown entry: it writes `fill_value` into every
    unknown cell of a new relation and fits the filler as if it had been observed.  Here every factor but the target's and
    every backbone stay frozen as there, and each iteration is the completion step of ``Dfmc`` (reference _dfmc.py:319-325:
    an unknown cell takes the current model's prediction) followed by the target's update (_dfmf.py:385-428) -- without the
    completed matrix: one pass per iteration over the known entries (SKF_REL_FOLD_CSR | SKF_REL_FOLD_KNOWN).

    Parameters as ``DfmfTransform``.  How a relation of the new graph enters:
    a ``Relation(scipy.sparse, ..., unstored='unknown')`` in any format scipy converts: as its known entries compressed
    along the target's side, never expanded, whatever its density; a ``MaskedArray`` with masked cells: as its unmasked
    cells, turned into the same lists on the host; stored / unmasked values that are not finite are unknown.  Anything with
    no unknown cell (an ndarray, a MaskedArray that masks nothing, ``unstored='zero'``) enters exactly as in
    ``DfmfTransform``: dense, or as its stored entries under the ``sparse_relations`` rule.  A relation with unknown cells
    AND a preprocessor raises ``DataFusionError`` (a preprocessor maps a matrix; there is none).
    `fill_value` is read by the initialiser only: it stands beneath the unknown cells where `random_c` / `random_vcol` form
    their column means (as in ``DfmfTransform``, same draws in the same order); the iterations never see it.
    n_run > 1 folds into the model of every restart on shared uploads, one restart after the other (no shared launches).
    `compute_err`, `stopping`, `stopping_system` read the KNOWN-ENTRY objective of such a relation, sum over its known
    entries of (v - x)^2 with the current target factor -- not the reference's norm of the working copy, which carries the
    previous iterate in the unknown cells (_dfmc.py:376-389).
    Completion with the new factor: ``DeviceCompleter`` with ``transformer.factor(target)``.
    """

    def _enter(self, relation, target, R, Theta):
        if not unknown_cells(relation):
            return super(DfmcTransform, self)._enter(relation, target, R, Theta)
        if relation.preprocessor:
            from ..base import DataFusionError
            raise DataFusionError('relation %s has unknown cells and a preprocessor: DfmcTransform folds in on the known '
                                  'entries alone and forms no matrix to preprocess' % (relation,))
        data = known_lists(relation, relation.row_type != target, float(self.fill_value))
        R.setdefault((relation.row_type, relation.col_type), []).append(data)
