"""`Dfmf(shard='owned')` on a scipy.sparse relation AND a scipy.sparse constraint over a real process group on the CPU: two
gloo ranks, the arithmetic in the host SIMT emulator.  Every rank hands its plan the CSR of its owned rows of both (never
``toarray()``), the library issues the exchanges through the callback communicator, and both ranks reproduce the oracle's
fit of the dense matrices to 1e-9."""
import os
import socket
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_USERS, N_MOVIES, RANKS = 120, 90, (16, 12, 4)
FIT = dict(max_iter=4, init_type='random', random_state=11, dtype='f64')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _graph(forbid):
    """users x movies counts and a constraint on the users as scipy.sparse (forbid: toarray() / todense() raise), or both as
    their ndarrays; movies x genres dense."""
    import sparse_dfmf_api_cases as AC
    import theta_csr_cases as TC
    from skfusion_amd.fusion import FusionGraph, Relation, ObjectType
    sp = AC.counts(N_USERS, N_MOVIES, 0.05, 3)
    coo, dense = TC.api_theta(N_USERS, 9)
    theta = coo.tocsr()
    if forbid:
        def refuse(*a, **k):
            raise AssertionError('an eligible sparse matrix was expanded')
        sp.toarray = sp.todense = theta.toarray = theta.todense = refuse
    rs = np.random.RandomState(1)
    users, movies, genres = ObjectType('users', RANKS[0]), ObjectType('movies', RANKS[1]), ObjectType('genres', RANKS[2])
    return FusionGraph([Relation(sp if forbid else sp.toarray(), users, movies, name='counts'),
                        Relation((rs.rand(N_MOVIES, 12) < 0.3).astype(float), movies, genres, name='genres'),
                        Relation(theta if forbid else dense, users, users, name='theta')])


def _worker(rank, world, port, out):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from skfusion_amd.fusion import Dfmf
    from skfusion_amd._engine import KnownEntries
    from emul.runtime import emulated_runtime, use_runtime
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        def refuse(*a, **k):
            raise AssertionError('a matrix given as its entries was expanded')
        KnownEntries.toarray = refuse
        with use_runtime(emulated_runtime()):
            g = _graph(forbid=True)
            fit = Dfmf(shard='owned', sparse_relations=True, sparse_constraints=True, **FIT).fuse(g)
            rels = [r for r in g.relations if r.row_type != r.col_type]
            arrs = [fit.factor(t) for t in g.object_types] + [fit.backbone(r) for r in rels]
        np.savez(os.path.join(out, 'owned%d.npz' % rank), *arrs)
    finally:
        dist.destroy_process_group()


def test_sparse_constraint_sharded_by_ownership_over_two_gloo_ranks(tmp_path):
    import torch.multiprocessing as mp
    from emul.runtime import build
    from helpers import relerr
    from oracle import dfmf_oracle as orc
    from skfusion_amd.fusion.decomposition.dfmf import graph_matrices, initial_factors
    build()                                   # compile once, before the workers race for it
    g = _graph(forbid=False)                  # the dense matrices, for the oracle
    types = list(g.object_types)
    rank = {t: int(t.rank) for t in types}
    R, Theta = graph_matrices(g, sparse_relations=False, sparse_constraints=False)
    assert len(Theta) == 1
    G0 = initial_factors(R, types, rank, FIT['init_type'], np.random.RandomState(FIT['random_state']), 1)[0]
    Go, So = orc.dfmf(R, Theta, types, rank, max_iter=FIT['max_iter'], G0=G0)
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    rels = [r for r in g.relations if r.row_type != r.col_type]
    for r in range(2):
        a = np.load(os.path.join(str(tmp_path), 'owned%d.npz' % r))
        for k, t in enumerate(types):
            assert relerr(a['arr_%d' % k], Go[t, t]) < 1e-9, (r, t.name)
        for k, rel in enumerate(rels):
            assert relerr(a['arr_%d' % (len(types) + k)], So[rel.row_type, rel.col_type][0]) < 1e-9, (r, rel.name)
