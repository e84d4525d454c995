"""Bind time and iteration rate of DFMF on a relation handed over as the CSR of its stored entries (SKF_REL_SPARSE_CSR,
unstored = zero) against the SAME data handed over as a dense matrix (the path a scipy.sparse relation took before:
toarray()), per engine and density.

    python tools/bench_sparse_dfmf.py [--iters 20] [--out profiles/r08_sparse_dfmf.txt]      the whole table
    python tools/bench_sparse_dfmf.py --one FORM DTYPE N_ROW N_COL PER_ROW RANK_ROW RANK_COL  one measurement (JSON line)

The table: 100 000 x 40 000, ranks 128 / 128, densities 1e-4, 1e-3, 1e-2 and 4/128 (the default rule
density * rank <= 4), CSR-fed and dense-fed, engines f64 / f32 / bf16; and 1 000 000 x 400 000 with 40 M entries, CSR
only (the dense form of it would be 800 GB as bf16).  Every measurement is a process of its own under its own
`timeout -k 10`; the first one that fails ends the run.  The dense form is assembled on the device (no n_i x n_j array
on the host).  Per measurement: plan creation + upload + bind (s), it/s as the median of 5 timed blocks after a
warm-up, workspace bytes."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def entries(n_r, n_c, per_row, seed=0):
    """per_row stored entries in every row, spread over the columns (strictly ascending by construction); values are
    multiples of 1/8 in (0, 8)."""
    from skfusion_amd._engine import KnownEntries
    rs = np.random.RandomState(seed)
    step = n_c // per_row
    cols = rs.randint(0, step, (n_r, per_row), dtype=np.int32)
    cols += (np.arange(per_row, dtype=np.int32) * step)[None, :]
    vals = rs.randint(1, 64, n_r * per_row, dtype=np.int32).astype(np.float64)
    vals /= 8.0
    return KnownEntries(np.arange(n_r + 1, dtype=np.int64) * per_row, cols.reshape(-1), vals, (n_r, n_c), unstored='zero')


def dense_on_device(ke, dtype):
    import torch
    from skfusion_amd._engine import device_matrix_from_tensor
    tdt = {'bf16': torch.bfloat16, 'f32': torch.float32, 'f64': torch.float64}[dtype]
    R = torch.zeros(ke.shape, dtype=tdt, device='cuda')
    rows = torch.from_numpy(ke.row_of_entries()).cuda()
    cols = torch.from_numpy(ke.indices.astype(np.int64)).cuda()
    R[rows, cols] = torch.from_numpy(ke.values).cuda().to(tdt)
    torch.cuda.synchronize()
    return device_matrix_from_tensor(R)


def one(form, dtype, n_r, n_c, per_row, c_r, c_c, iters):
    import __graft_entry__
    __graft_entry__.build()
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DevicePlan
    ke = entries(n_r, n_c, per_row)
    data = ke if form == 'csr' else dense_on_device(ke, dtype)
    types, n, ranks = ['row', 'col'], {'row': n_r, 'col': n_c}, {'row': c_r, 'col': c_c}
    t0 = time.perf_counter()
    plan = DevicePlan(types, n, ranks, [('row', 'col', data, None)], [], nat.SKF_DFMF, dtype=dtype)
    plan.synchronize()
    t1 = time.perf_counter()
    try:
        rs = np.random.RandomState(1)
        for t in types:
            plan.set_factor(t, rs.rand(n[t], ranks[t]) * 0.1 + 0.01)
        plan.iterate(3)                                  # warm-up
        plan.synchronize()
        rates = []
        for _ in range(5):
            t2 = time.perf_counter()
            plan.iterate(iters)
            plan.synchronize()
            rates.append(iters / (time.perf_counter() - t2))
        err = plan.relation_sqerr(0)
        out = dict(form=form, dtype=dtype, shape=[n_r, n_c], entries=n_r * per_row, density=per_row / float(n_c),
                   ranks=[c_r, c_c], create_upload_bind_s=round(t1 - t0, 3), it_per_s=round(float(np.median(rates)), 2),
                   it_per_s_min=round(min(rates), 2), it_per_s_max=round(max(rates), 2),
                   workspace_bytes=plan.workspace_bytes, sqerr=err)
    finally:
        plan.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--dtypes', default='bf16,f32,f64')
    ap.add_argument('--skip-big', action='store_true')
    ap.add_argument('--one', nargs=7, metavar=('FORM', 'DTYPE', 'N_ROW', 'N_COL', 'PER_ROW', 'RANK_ROW', 'RANK_COL'))
    a = ap.parse_args()
    if a.one:
        one(a.one[0], a.one[1], *[int(v) for v in a.one[2:]], iters=a.iters)
        return
    jobs = []
    for dtype in a.dtypes.split(','):
        for per_row in (4, 40, 400, 1250):               # 1e-4, 1e-3, 1e-2, 4/128 of 40 000 columns
            for form in ('csr', 'dense'):
                jobs.append((form, dtype, 100000, 40000, per_row, 128, 128, 300))
    if not a.skip_big:
        jobs.append(('csr', 'bf16', 1000000, 400000, 40, 128, 64, 600))
    lines = []
    for form, dtype, n_r, n_c, per_row, c_r, c_c, limit in jobs:     # every measurement: its own process, its own time limit
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--iters', str(a.iters), '--one',
               form, dtype, str(n_r), str(n_c), str(per_row), str(c_r), str(c_c)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if done.returncode != 0:
            print('measurement %r ended with status %d: stopping here' % (cmd[8:], done.returncode), flush=True)
            break
        line = [l for l in done.stdout.splitlines() if l.startswith('{')][-1]
        print(line, flush=True)
        lines.append(json.loads(line))
    if a.out:
        with open(a.out, 'a') as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + '\n')
    sys.exit(0 if len(lines) == len(jobs) else 1)


if __name__ == '__main__':
    main()
