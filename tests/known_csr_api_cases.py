"""Relations given as scipy.sparse matrices through the public API (Relation(..., unstored=...)): the list path of Dfmc
against the MaskedArray the relation means, and the expansions everywhere else -- shared by the emulator (small) and
the GPU (larger) tests."""
import numpy as np
import scipy.sparse

from skfusion_amd.fusion import FusionGraph, Relation, ObjectType, Dfmc, Dfmf
from helpers import relerr


def ratings(n_u, n_m, share, seed, nonfinite=False):
    """A ratings relation as COO triplets (with a duplicate and a stored zero) and its MaskedArray equivalent."""
    rs = np.random.RandomState(seed)
    k = int(share * n_u * n_m)
    u, m = rs.randint(0, n_u, k), rs.randint(0, n_m, k)
    v = (np.floor(rs.rand(k) * 10.0) + 1.0) / 10.0
    u = np.concatenate([u, [0, 0]])
    m = np.concatenate([m, [1, 1]])                     # the same cell twice: summed
    v = np.concatenate([v, [0.3, 0.4]])
    u = np.concatenate([u, [2]])
    m = np.concatenate([m, [3]])
    v = np.concatenate([v, [0.0]])                      # a stored zero: a known zero
    if nonfinite:
        u = np.concatenate([u, [4, 5]])
        m = np.concatenate([m, [2, 7]])
        v = np.concatenate([v, [np.nan, np.inf]])       # stored non-finite values: the fill beneath, still known
    csr = scipy.sparse.coo_matrix((v, (u, m)), shape=(n_u, n_m)).tocsr()
    dense = csr.toarray()                               # (the equivalent of the matrix handed over: its sums of duplicates)
    known = np.zeros((n_u, n_m), dtype=bool)
    known[u, m] = True
    if nonfinite:                                       # (toarray sums the NaN / inf into their cells as they are)
        dense[4, 2], dense[5, 7] = np.nan, np.inf
    return csr, np.ma.MaskedArray(dense, mask=~known)


def graph(rat, n_g=12, ranks=(16, 12, 4), seed=1, **kw):
    """users x movies ratings (sparse or masked) + a dense movies x genres relation."""
    rs = np.random.RandomState(seed)
    n_u, n_m = rat.shape
    users, movies, genres = ObjectType('users', ranks[0]), ObjectType('movies', ranks[1]), ObjectType('genres', ranks[2])
    rels = [Relation(rat, users, movies, name='ratings', **kw),
            Relation((rs.rand(n_m, n_g) < 0.3).astype(float), movies, genres, name='genres')]
    return FusionGraph(rels), users, movies


def fit(cls, g, **kw):
    return cls(**kw).fuse(g)


def same_fit(a, b, ga, gb, exact=True, tol=0.0):
    worst = 0.0
    for ta, tb in zip(ga.object_types, gb.object_types):
        fa, fb = a.factor(ta), b.factor(tb)
        assert fa.shape == fb.shape
        if exact:
            assert np.array_equal(fa, fb), 'factor of %s differs' % ta
        worst = max(worst, relerr(fa, fb))
    for ra, rb in zip(ga.relations, gb.relations):
        if exact:
            assert np.array_equal(a.backbone(ra), b.backbone(rb))
        worst = max(worst, relerr(a.backbone(ra), b.backbone(rb)))
    assert worst <= tol, worst
    return worst


def list_path_equals_mask_form(monkeypatch, n_u, n_m, share, dtype, max_iter, tmp_path=None, **kw):
    """init 'random' (or G0 drawn from the same stream): bit for bit the MaskedArray fit on the list path."""
    monkeypatch.setenv('SKF_DFMC_SPARSE', '1')           # the mask form takes the lists too
    csr, ma = ratings(n_u, n_m, share, 7)
    gs, us, ms = graph(csr, unstored='unknown')
    gm, um, mm = graph(ma)
    a = fit(Dfmc, gs, max_iter=max_iter, init_type='random', random_state=0, dtype=dtype, **kw)
    b = fit(Dfmc, gm, max_iter=max_iter, init_type='random', random_state=0, dtype=dtype, **kw)
    same_fit(a, b, gs, gm)
    rel_s, rel_m = list(gs.relations)[0], list(gm.relations)[0]
    assert np.array_equal(a.complete(rel_s), b.complete(rel_m))          # shapes and factors only
    assert [list(map(str, p)) for p in a.chain(us, ms)] == [list(map(str, p)) for p in b.chain(um, mm)]
    if tmp_path is not None:
        path = str(tmp_path / 'fit.npz')
        a.save(path)
        loaded = type(a).load(path, gs)
        assert np.array_equal(loaded.complete(rel_s), a.complete(rel_s))
    return a, b


def nonfinite_with_constant_fill(monkeypatch, n_u, n_m, dtype, max_iter):
    monkeypatch.setenv('SKF_DFMC_SPARSE', '1')
    csr, ma = ratings(n_u, n_m, 0.05, 8, nonfinite=True)
    gs, _, _ = graph(csr, unstored='unknown', fill_value=0.25)
    gm, _, _ = graph(ma, fill_value=0.25)
    same_fit(fit(Dfmc, gs, max_iter=max_iter, init_type='random', random_state=3, dtype=dtype),
             fit(Dfmc, gm, max_iter=max_iter, init_type='random', random_state=3, dtype=dtype), gs, gm)


def column_initialisers(monkeypatch, n_u, n_m, init_type, dtype, max_iter, tol_fit):
    """random_c / random_vcol from the entries: G0 within 1e-13 of the dense statistics, the fit within tol_fit.  (random_c
    with fill 'mean' is left out: its column ranking breaks near-ties by the last bit of the mean, which the entries give
    as a sum in another order than NumPy's pairwise sum over the dense matrix.)"""
    from skfusion_amd.fusion.decomposition.dfmf import graph_matrices, initial_factors
    monkeypatch.setenv('SKF_DFMC_SPARSE', '1')
    csr, ma = ratings(n_u, n_m, 0.05, 9)
    for fill in ((0.5,) if init_type == 'random_c' else ('mean', 0.5)):
        gs, _, _ = graph(csr, unstored='unknown', fill_value=fill)
        gm, _, _ = graph(ma, fill_value=fill)
        Rs = graph_matrices(gs, with_masks=True, known_entries=True)[0]
        Rm = graph_matrices(gm, with_masks=True)[0]
        G0s = initial_factors(Rs, list(gs.object_types), {t: t.rank for t in gs.object_types}, init_type,
                              np.random.RandomState(4), 2)
        G0m = initial_factors(Rm, list(gm.object_types), {t: t.rank for t in gm.object_types}, init_type,
                              np.random.RandomState(4), 2)
        for ks, km in zip(G0s, G0m):
            for (ts, _), (tm, _) in zip(ks, km):
                assert relerr(ks[ts, ts], km[tm, tm]) <= 1e-13
        same_fit(fit(Dfmc, gs, max_iter=max_iter, init_type=init_type, random_state=4, dtype=dtype),
                 fit(Dfmc, gm, max_iter=max_iter, init_type=init_type, random_state=4, dtype=dtype), gs, gm,
                 exact=False, tol=tol_fit)


def several_runs(monkeypatch, n_u, n_m, dtype, max_iter, n_jobs):
    monkeypatch.setenv('SKF_DFMC_SPARSE', '1')
    csr, ma = ratings(n_u, n_m, 0.05, 10)
    gs, _, _ = graph(csr, unstored='unknown')
    gm, _, _ = graph(ma)
    kw = dict(max_iter=max_iter, init_type='random', random_state=5, dtype=dtype, n_run=3, n_jobs=n_jobs)
    a, b = fit(Dfmc, gs, **kw), fit(Dfmc, gm, **kw)
    for run in range(3):
        for ta, tb in zip(gs.object_types, gm.object_types):
            assert np.array_equal(a.factor(ta, run), b.factor(tb, run))
        for ra, rb in zip(gs.relations, gm.relations):
            assert np.array_equal(a.backbone(ra, run), b.backbone(rb, run))


def expanded_cases(n_u, n_m, dtype, max_iter):
    """Where the lists do not apply, the relation is its MaskedArray: row_mean, Dfmf, a preprocessor, shard='rows'
    (one process), and unstored='zero' is scipy's own toarray()."""
    csr, ma = ratings(n_u, n_m, 0.05, 11)
    kw = dict(max_iter=max_iter, init_type='random_vcol', random_state=6, dtype=dtype)
    for cls, rkw, fkw in ((Dfmc, dict(fill_value='row_mean'), {}), (Dfmf, {}, {}),
                          (Dfmc, dict(preprocessor=lambda x: x * 2.0), {}), (Dfmc, {}, dict(shard='rows'))):
        gs, _, _ = graph(csr, unstored='unknown', **rkw)
        gm, _, _ = graph(ma, **rkw)
        same_fit(fit(cls, gs, **dict(kw, **fkw)), fit(cls, gm, **dict(kw, **fkw)), gs, gm)
    gz, _, _ = graph(csr)                                              # unstored='zero' (default)
    gd, _, _ = graph(csr.toarray())
    same_fit(fit(Dfmc, gz, **kw), fit(Dfmc, gd, **kw), gz, gd)
    same_fit(fit(Dfmf, gz, **kw), fit(Dfmf, gd, **kw), gz, gd)
