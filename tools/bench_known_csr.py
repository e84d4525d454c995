"""Bind time, iteration rate and host memory of DFMC on a ratings relation handed over as its known entries
(SKF_REL_KNOWN_CSR) against the same data handed over as dense data + mask.  Both build the same lists (the mask form
with SKF_DFMC_SPARSE=1), so the iterations should cost the same; what differs is everything before the first one.

    python tools/bench_known_csr.py [--iters 20] [--skip-mask]

One JSON line per measurement: form, shape, known entries, host preparation (s), plan creation + upload + bind (s),
it/s over --iters iterations, workspace bytes, peak RSS of the process so far (GB).  The config-5 shape (100k x 40k,
2 % known) is measured in the CSR form only: the mask form of it needs >= 36 GB of host memory."""
import argparse
import json
import os
import resource
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

__graft_entry__.build()
import skfusion_amd._native as nat  # noqa: E402
from skfusion_amd._engine import DevicePlan, KnownEntries  # noqa: E402


def ratings(n_u, n_m, per_row, seed=0):
    """per_row known entries in every row, spread uniformly over the columns (strictly ascending by construction)."""
    rs = np.random.RandomState(seed)
    step = n_m // per_row
    cols = rs.randint(0, step, (n_u, per_row), dtype=np.int32)
    cols += (np.arange(per_row, dtype=np.int32) * step)[None, :]
    vals = rs.randint(1, 11, n_u * per_row, dtype=np.int32).astype(np.float64)
    vals /= 10.0
    return KnownEntries(np.arange(n_u + 1, dtype=np.int64) * per_row, cols.reshape(-1), vals, (n_u, n_m))


def peak_gb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2.0 ** 20


def measure(form, n_u, n_m, per_row, rank, iters, dtype='bf16'):
    t0 = time.perf_counter()
    ke = ratings(n_u, n_m, per_row)
    rel = ('user', 'movie', ke, None)
    if form == 'mask':
        rel = ('user', 'movie', ke.toarray(0.0).astype(np.float32), ke.mask())
        del ke
    t1 = time.perf_counter()
    types, n, ranks = ['user', 'movie'], {'user': n_u, 'movie': n_m}, {'user': rank, 'movie': rank}
    plan = DevicePlan(types, n, ranks, [rel], [], nat.SKF_DFMC, dtype=dtype)
    plan.synchronize()
    t2 = time.perf_counter()
    del rel
    try:
        rs = np.random.RandomState(1)
        for t in types:
            plan.set_factor(t, rs.rand(n[t], rank) * 0.1 + 0.01)
        plan.iterate(2)                                  # warm-up
        plan.synchronize()
        t3 = time.perf_counter()
        plan.iterate(iters)
        plan.synchronize()
        t4 = time.perf_counter()
        out = dict(form=form, shape=[n_u, n_m], known=n_u * per_row, rank=rank, dtype=dtype,
                   host_prep_s=round(t1 - t0, 3), create_upload_bind_s=round(t2 - t1, 3),
                   it_per_s=round(iters / (t4 - t3), 2), workspace_bytes=plan.workspace_bytes,
                   peak_rss_gb=round(peak_gb(), 2))
    finally:
        plan.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-mask', action='store_true')
    a = ap.parse_args()
    os.environ['SKF_DFMC_SPARSE'] = '1'                  # the mask form takes the lists at every share
    measure('csr', 100000, 40000, 800, 128, a.iters)     # config 5
    # the largest mask form measured here: 25k x 20k (500 M cells; f32 data + bool mask = 2.5 GB on the host)
    measure('csr', 25000, 20000, 400, 128, a.iters)
    if not a.skip_mask:
        measure('mask', 25000, 20000, 400, 128, a.iters)


if __name__ == '__main__':
    main()
