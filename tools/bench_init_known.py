"""Time of the column-mean initialisers on a relation with MISSING values kept as lists -- the DFMC known-entry lists
(SKF_REL_KNOWN_CSR) of BASELINE config 5: 100 000 x 40 000, 800 known entries in every row (80 M), rank 256 both ways -- on
the device (skf_plan_relation_norms_filled, skf_plan_init_column_means_filled) against the host initialiser
(`_init._KnownView`), which walks the entries once per factor column and fills one dense column buffer per column.

    python tools/bench_init_known.py [--scales 10,1] [--dtypes bf16,f32] [--hubs 0] [--no-host]
    python tools/bench_init_known.py --host-only [--shape 20000,8000,80]      # no GPU, no library: the host rates alone

One JSON line per measurement:
  where 'device': draw_s (the index shuffles on the host: the random stream, which stays there), pools_s (`random_c` only:
        the norm pass, its read-back, square roots and the stable sorts), init_s (selections up, the flags, the list passes
        with their epilogue, skf_set_factor, one synchronisation: `DeviceInit.apply` once the pools exist), norms_s (the norm
        pass alone, read-back included), work = `init_known_work`'s count.
  where 'host': seconds of `_init.initialize` on the same entries (1/10 linear scale only; the full size is extrapolated by
        the reader and must say so).
  where 'host-rates' (--host-only): `_KnownView.column_norms()` in dense cells per second and `row_means()` in entries per
        second, both orientations -- what INIT_KNOWN_MIN of fusion/decomposition/dfmf.py is set by.
--hubs H: the first H column buckets hold ONE column each, stored by every row -- lines of n_rows entries in the transposed
view (a popular item), which the list pass runs serially in their wave."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL = (100000, 40000, 800)         # rows, columns, known entries per row
RANK = 256
TYPES = ['user', 'movie']


def ratings(n_u, n_m, per_row, hubs=0, seed=0):
    """per_row known entries in every row, one per bucket of n_m // per_row columns (strictly ascending by construction);
    ratings 0.5 .. 5; the fill beneath the unknown entries is 2.5."""
    from skfusion_amd._engine import KnownEntries
    rs = np.random.RandomState(seed)
    step = n_m // per_row
    cols = rs.randint(0, step, (n_u, per_row), dtype=np.int32)
    cols[:, :hubs] = 0
    cols += (np.arange(per_row, dtype=np.int32) * step)[None, :]
    vals = rs.randint(1, 11, n_u * per_row, dtype=np.int32).astype(np.float64)
    vals /= 2.0
    return KnownEntries(np.arange(n_u + 1, dtype=np.int64) * per_row, cols.reshape(-1), vals, (n_u, n_m), fill=2.5)


def work(n_u, n_m, nnz, init_type):
    return nnz * 2 * RANK + (2 * n_u * n_m if init_type == 'random_c' else 0)


def device(scale, dtype, init_type, hubs):
    import __graft_entry__
    __graft_entry__.build()
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DevicePlan
    from skfusion_amd.fusion.decomposition import _init
    n_u, n_m, per_row = FULL[0] // scale, FULL[1] // scale, FULL[2] // scale
    ke = ratings(n_u, n_m, per_row, hubs)
    n, ranks = {'user': n_u, 'movie': n_m}, {'user': RANK, 'movie': RANK}
    plan = DevicePlan(TYPES, n, ranks, [('user', 'movie', ke, None)], [], nat.SKF_DFMC, dtype=dtype)
    plan.synchronize()
    try:
        shapes = {('user', 'movie'): (n_u, n_m)}
        out = dict(where='device', scale=scale, dtype=dtype, init_type=init_type, hubs=hubs, shape=[n_u, n_m], known=ke.known,
                   work=work(n_u, n_m, ke.known, init_type))
        for rep in ('warm', 'timed'):                          # (the first pass pays the code-object loads)
            rs = np.random.RandomState(0)
            t0 = time.perf_counter()
            di = _init.DeviceInit(_init.draw_positions(TYPES, ranks, shapes, init_type, rs), init_type, {})
            t1 = time.perf_counter()
            if init_type == 'random_c':
                di._pool(plan, 0, (('user', 'movie'), False))
            t2 = time.perf_counter()
            di.apply(plan, TYPES)
            t3 = time.perf_counter()
            plan.relation_norms(0)
            t4 = time.perf_counter()
        out.update(draw_s=round(t1 - t0, 4), pools_s=round(t2 - t1, 4), init_s=round(t3 - t2, 4), norms_s=round(t4 - t3, 4),
                   device_total_s=round(t3 - t1, 4))
        assert np.isfinite(plan.get_factor('user')).all()
    finally:
        plan.close()
    print(json.dumps(out), flush=True)


def host(scale, init_type, hubs):
    from skfusion_amd.fusion.decomposition import _init
    n_u, n_m, per_row = FULL[0] // scale, FULL[1] // scale, FULL[2] // scale
    ke = ratings(n_u, n_m, per_row, hubs)
    n, ranks = {'user': n_u, 'movie': n_m}, {'user': RANK, 'movie': RANK}
    t0 = time.perf_counter()
    _init.initialize(TYPES, n, ranks, {('user', 'movie'): ke}, init_type, np.random.RandomState(0), {})
    dt = time.perf_counter() - t0
    w = work(n_u, n_m, ke.known, init_type)
    print(json.dumps(dict(where='host', scale=scale, init_type=init_type, shape=[n_u, n_m], known=ke.known, work=w,
                          host_s=round(dt, 3), work_per_s=round(w / dt, 1))), flush=True)


def host_rates(n_u, n_m, per_row):
    """The two terms of the host initialiser's cost on this machine's CPU, per orientation."""
    from skfusion_amd.fusion.decomposition import _init
    ke = ratings(n_u, n_m, per_row)
    for transposed in (False, True):
        view = _init._KnownView(ke, transposed)
        t0 = time.perf_counter()
        view.column_norms()
        t1 = time.perf_counter()
        columns = np.random.RandomState(1).permutation(view.shape[1])[:int(.2 * view.shape[1])]
        reps = 5
        for _ in range(reps):
            view.row_means(columns)
        t2 = time.perf_counter()
        print(json.dumps(dict(where='host-rates', shape=[n_u, n_m], known=ke.known, transposed=transposed,
                              column_norms_s=round(t1 - t0, 3), cells_per_s=round(n_u * n_m / (t1 - t0), 1),
                              row_means_s=round((t2 - t1) / reps, 4), entries_per_s=round(ke.known * reps / (t2 - t1), 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', default='10,1')
    ap.add_argument('--dtypes', default='bf16,f32')
    ap.add_argument('--hubs', type=int, default=0)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--host-only', action='store_true', help='the host rates alone: needs neither a GPU nor the library')
    ap.add_argument('--shape', default='20000,8000,80', help='--host-only: rows, columns, known entries per row')
    a = ap.parse_args()
    if a.host_only:
        host_rates(*[int(v) for v in a.shape.split(',')])
        return
    for scale in [int(s) for s in a.scales.split(',')]:
        for dtype in a.dtypes.split(','):
            for init_type in ('random_vcol', 'random_c'):
                device(scale, dtype, init_type, a.hubs)
        if scale > 1 and not a.no_host:
            for init_type in ('random_vcol', 'random_c'):
                host(scale, init_type, a.hubs)


if __name__ == '__main__':
    main()
