"""DFMC on relations handed over as their known entries (SKF_REL_KNOWN_CSR, skf_plan_set_known_entries) against the same
relations handed over as dense data + mask -- the SAME cases on the host emulator and on the GPU.  Both forms build the
known-entry lists of csrc/skf_known.h (the mask form with SKF_DFMC_SPARSE=1), byte for byte the same lists, so every
iteration after bind must agree bit for bit."""
import numpy as np

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, KnownEntries, pack_mask

import known_cases as K


def known_entries_of(R, M):
    """Dense relation + mask (True = unknown) -> KnownEntries holding exactly its known entries."""
    known = ~np.asarray(M, dtype=bool)
    rows, cols = np.nonzero(known)                      # row-major: columns ascending within a row
    indptr = np.zeros(R.shape[0] + 1, dtype=np.int64)
    np.cumsum(known.sum(axis=1), out=indptr[1:])
    return KnownEntries(indptr, cols, np.asarray(R, dtype=np.float64)[rows, cols], R.shape)


def edited_graph(n, ranks, known_share, seed, edits):
    """known_cases.masked_graph with the mask of the ratings relation edited: 'empty' (an empty row and column),
    'full_row' (one row entirely known), 'none' (nothing known at all)."""
    types, rels, thetas, G0 = K.masked_graph(n, ranks, known_share, seed)
    i, j, R, M = rels[0]
    M = M.copy()
    if 'empty' in edits:
        M[3, :] = True
        M[:, 5] = True
    if 'full_row' in edits:
        M[7, :] = False
    if 'none' in edits:
        M[:] = True
    rels[0] = (i, j, R, M)
    return types, rels, thetas, G0


def run_plan(types, n, ranks, rels, thetas, G0, dtype, iters):
    plan = DevicePlan(types, n, ranks, rels, thetas, nat.SKF_DFMC, dtype=dtype)
    try:
        for t in types:
            plan.set_factor(t, G0[t])
        errs = []
        for _ in range(iters):
            plan.iterate(1)
            errs.append([plan.relation_sqerr(k) for k in range(len(rels))])
        G = {t: plan.get_factor(t) for t in types}
        S = [plan.get_backbone(k) for k in range(len(rels))]
        return G, S, np.array(errs), plan.workspace_bytes
    finally:
        plan.close()


def csr_against_mask(n, ranks, known_share, dtype, parts, monkeypatch, seed=0, edits=(), iters=3):
    """Both masked relations of the graph fed as known entries vs fed as dense + mask: G, S and every squared error
    np.array_equal; the CSR-fed workspace smaller by at least the packed masks it never holds."""
    monkeypatch.setenv('SKF_DFMC_SPARSE', '1')
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    types, rels, thetas, G0 = edited_graph(n, ranks, known_share, seed, edits)
    mem = nat.get_runtime().mem
    mask_rels, csr_rels = [], []
    mb_bytes = 0
    for (i, j, R, M) in rels:
        if M is None:
            mask_rels.append((i, j, R, None))
            csr_rels.append((i, j, R, None))
            continue
        pm = pack_mask(M, mem)
        pm.known = max(pm.known, 1)        # (a bound, not a count: with nothing known the mask form still takes lists)
        mask_rels.append((i, j, R, pm))
        csr_rels.append((i, j, known_entries_of(R, M), None))
        mb_bytes += R.shape[0] * ((R.shape[1] + 127) // 128 * 16)
    Gm, Sm, Em, wm = run_plan(types, n, ranks, mask_rels, thetas, G0, dtype, iters)
    Gc, Sc, Ec, wc = run_plan(types, n, ranks, csr_rels, thetas, G0, dtype, iters)
    for t in types:
        assert np.array_equal(Gc[t], Gm[t]), 'G_%s: CSR-fed differs from mask-fed' % t
        assert np.isfinite(Gc[t]).all()
    for k in range(len(rels)):
        assert np.array_equal(Sc[k], Sm[k]), 'S_%d: CSR-fed differs from mask-fed' % k
    assert np.array_equal(Ec, Em), 'squared errors: CSR-fed differs from mask-fed'
    assert wc <= wm - mb_bytes, 'workspace: CSR-fed %d B, mask-fed %d B, packed masks %d B' % (wc, wm, mb_bytes)
    return Gc, Sc, Ec


# ---- refusal order: every user of the shared CSR check answers after that one kernel -----------------------------------
DEFECTS = ('range', 'descending', 'indptr')


def small_lists(which):
    """Six entries of a 4 x 6 relation as CSR: canonical ('ok'), or with a column out of range, a descending pair, or a
    backward indptr step (the lists of test_invalid_lists_are_refused_before_any_gather)."""
    indptr = np.array([0, 2, 4, 4, 6], dtype=np.int64)
    idx = np.array([1, 3, 0, 2, 4, 5], dtype=np.int32)
    if which == 'range':
        idx[3] = 6                                      # column 6 of 6
    elif which == 'descending':
        idx[2], idx[3] = 2, 0
    elif which == 'indptr':
        indptr[2] = 1                                   # 2 -> 1 -> 4: a negative step
    else:
        assert which == 'ok'
    return indptr, idx


def small_plan(which, variant, unstored, target=None):
    """A plan of 4 x 6 objects, ranks 2, whose only relation is small_lists(which), already on the device (no host check)."""
    from skfusion_amd._engine import DeviceKnownEntries
    indptr, idx = small_lists(which)
    mem = nat.get_runtime().mem
    dev = DeviceKnownEntries(mem.from_host(indptr), mem.from_host(idx), mem.from_host(np.random.RandomState(0).rand(6)), (4, 6), 6,
                             unstored=unstored)
    return DevicePlan(['a', 'b'], {'a': 4, 'b': 6}, {'a': 2, 'b': 2}, [('a', 'b', dev, None)], [], variant, target=target)


def refused_after_one_launch(call, which):
    """`call(which)` with defective lists ends in SKF_E_INVALID after exactly one kernel launch -- the validation, nothing
    that gathers through the lists --, and the same call with the canonical lists succeeds afterwards."""
    import pytest
    from skfusion_amd._engine import launch_count
    before = launch_count()
    with pytest.raises(nat.SkfNativeError) as err:
        call(which)
    assert err.value.code == nat.SKF_E_INVALID
    assert launch_count() - before == 1
    call('ok')
