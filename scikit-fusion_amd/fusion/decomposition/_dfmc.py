"""Functional solver seam of DFMC -- same signature as the reference's ``dfmc()``
(_dfmc.py:181-184).  ``M[(i,j)]`` is a list (parallel to ``R[(i,j)]``) of boolean masks or
``None``; masked entries are unknown and are re-estimated from the current model in every
iteration (_dfmc.py:287-292, :319-325).  The relation matrices passed in are never modified
(the engine completes a device-side copy)."""
from ... import _native as nat
from ._dfmf import run_fit, run_fit_sharded, run_fit_rows, run_fit_owned, refuse_constraint_entries, _fit_by_shard      # noqa: F401


def _expand_known_entries(R, M):
    """Relations given as their known entries (_engine.KnownEntries) -> their mask form (dense data + mask)."""
    from ..._engine import KnownEntries
    R2, M2 = {}, {}
    for key, mats in R.items():
        masks = (M or {}).get(key) or [None] * len(mats)
        R2[key] = [m.toarray() if isinstance(m, KnownEntries) else m for m in mats]
        M2[key] = [m.mask() if isinstance(m, KnownEntries) and m.unstored != 'zero' else (None if isinstance(m, KnownEntries) else mk)
                   for m, mk in zip(mats, masks)]
    return R2, M2


def dfmc(R, M, Theta, obj_types, obj_type2rank, max_iter=10, init_type="random_vcol",
         stopping=None, stopping_system=None, verbose=0, compute_err=False, callback=None,
         random_state=None, n_jobs=1, dtype='f64', G0=None, engine=None, shard=None, sparse_constraints=False, validation=None):
    """Data fusion by matrix completion -- drop-in for reference ``dfmc`` (_dfmc.py:181).  Constraints given as their entries:
    as in ``_dfmf.dfmf`` (shard None / 'runs'; shard='owned' with ``sparse_constraints=True``); ``validation``: as there."""
    if shard in ('relations', 'rows'):          # (an ownership-sharded fit slices the entries by rows; these take the mask form)
        R, M = _expand_known_entries(R, M)
    return _fit_by_shard(nat.SKF_DFMC, R, M, Theta, obj_types, obj_type2rank, max_iter, init_type, stopping,
                         stopping_system, verbose, compute_err, callback, random_state, dtype, G0, engine, shard,
                         sparse_constraints, validation)
