"""``Dfmc`` -- data fusion by matrix completion, class layer of the drop-in boundary
(reference ``skfusion/fusion/decomposition/dfmc.py:18-115``).  Masked entries of a relation
(numpy masked arrays that are still masked after fill + preprocess) are treated as unknown
and completed by the model; the relation objects' data is never modified."""
from . import _dfmc
from .dfmf import _Fuser

__all__ = ['Dfmc']


class Dfmc(_Fuser):
    """Parameters identical to the reference: max_iter=100, init_type='random_c', n_run=1,
    stopping=None, stopping_system=None, verbose=0, compute_err=False, callback=None,
    random_state=None, n_jobs=1.  Addition: dtype='f64' | 'f32'.  A relation given as its known entries
    (``Relation(scipy.sparse matrix, ..., unstored='unknown')``) is fitted on those entries alone with shard='runs'
    (see ``Relation``) and with shard='owned', where every rank uploads the known entries of its owned rows only (the
    whole matrix stays on every process's host for the initialisers; 'rows' / 'relations' expand it); such a relation with
    fill_value 'row_mean' / 'col_mean' (no mask is left) as entries plus rank one with shard='runs' (``sparse_relations``,
    ``filled_entries_apply``); one whose unstored entries are zero on its stored entries (``sparse_relations``, see ``Dfmf``); a
    ``scipy.sparse`` constraint as its entries (``sparse_constraints``, see ``Dfmf``)."""

    _variant = 'dfmc'
    _keeps_masks = True
    _takes_known_entries = True
    _shares_launches = False    # (the restarts of a Dfmc fit have no shared-launch branch)

    def __init__(self, max_iter=100, init_type='random_c', n_run=1, stopping=None,
                 stopping_system=None, verbose=0, compute_err=False, callback=None,
                 random_state=None, n_jobs=1, dtype='f64', shard='runs', device_fill=False, sparse_relations=None,
                 sparse_constraints=None, init_device=None):
        super(Dfmc, self).__init__()
        self._set_params(vars())

    def _solve(self, M, **kw):
        return _dfmc.dfmc(M=M, **kw)
