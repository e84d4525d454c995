"""Iteration rate, HBM workspace and host peak RSS of a DFMF fit on a ratings-like relation with MISSING values, handed over
as entries plus rank one (SKF_REL_FILL_RANK1: the filled matrix is a b^T + D, never expanded) against the SAME filled matrix
handed over dense -- the path such a relation took before (Relation.filled() of the MaskedArray, then the dense contraction).

    python tools/bench_filled_entries.py [--iters 20] [--out profiles/r17_filled_entries.txt]     the whole table
    python tools/bench_filled_entries.py --one FORM DTYPE FILL N_ROW N_COL PER_ROW RANK_ROW RANK_COL    one measurement (JSON line)

The table: BASELINE config 5's ratings relation -- 100 000 x 40 000, 2 % known (800 per row), ranks 128 / 256 -- with
fill 'mean' and 'row_mean', engines bf16 and f32, entries-fed and dense-fed.  Every measurement is a process of its own
under its own `timeout -k 10`; the first one that fails ends the run.  The dense form is assembled ON THE DEVICE (a b^T,
then the stored values scattered in), so its host RSS is NOT what the class layer paid for it before: Relation.filled()
formed the n_i x n_j float64 array on the host, 32 GB at this size; the figure recorded for the dense form is the device
side only.  Per measurement: plan creation + upload + bind (s), it/s as the median of 5 timed blocks after a warm-up,
workspace bytes, device bytes of the relation as handed over, peak RSS of the process."""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ratings(n_r, n_c, per_row, fill, seed=0):
    """per_row stored ratings in every row but one (row 7 holds none), spread over the columns (strictly ascending by
    construction); values are multiples of 1/2 in [1/2, 5].  The fill vectors as Relation.filled_entries() forms them."""
    from skfusion_amd._engine import KnownEntries
    rs = np.random.RandomState(seed)
    step = n_c // per_row
    cols = rs.randint(0, step, (n_r, per_row), dtype=np.int32)
    cols += (np.arange(per_row, dtype=np.int32) * step)[None, :]
    vals = rs.randint(1, 11, (n_r, per_row)).astype(np.float64) / 2.0
    count = np.full(n_r, per_row, dtype=np.int64)
    count[7] = 0
    keep = np.repeat(count > 0, per_row)
    indptr = np.zeros(n_r + 1, dtype=np.int64)
    np.cumsum(count, out=indptr[1:])
    cols, vals = cols.reshape(-1)[keep], vals.reshape(-1)[keep]
    m = vals.sum() / vals.size
    a, b = np.ones(n_r), np.ones(n_c)
    if fill == 'mean':
        a[:] = m
    elif fill == 'row_mean':
        a = np.where(count > 0, np.add.reduceat(vals, np.minimum(indptr[:-1], vals.size - 1)) / np.maximum(count, 1), m)
    else:
        raise ValueError(fill)
    return KnownEntries(indptr, cols, vals, (n_r, n_c), unstored='zero', row_fill=a, col_fill=b)


def dense_on_device(ke, dtype):
    import torch
    from skfusion_amd._engine import device_matrix_from_tensor
    tdt = {'bf16': torch.bfloat16, 'f32': torch.float32, 'f64': torch.float64}[dtype]
    a = torch.from_numpy(ke.row_fill).cuda()
    b = torch.from_numpy(ke.col_fill).cuda()
    R = torch.empty(ke.shape, dtype=tdt, device='cuda')
    block = 4096
    for r0 in range(0, ke.shape[0], block):              # (no n_i x n_j f64 temporary on the device either)
        R[r0:r0 + block] = torch.outer(a[r0:r0 + block], b).to(tdt)
    rows = torch.from_numpy(ke.row_of_entries()).cuda()
    cols = torch.from_numpy(ke.indices.astype(np.int64)).cuda()
    R[rows, cols] = torch.from_numpy(ke.values).cuda().to(tdt)
    torch.cuda.synchronize()
    return device_matrix_from_tensor(R)


def one(form, dtype, fill, n_r, n_c, per_row, c_r, c_c, iters):
    import __graft_entry__
    __graft_entry__.build()
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DevicePlan
    ke = ratings(n_r, n_c, per_row, fill)
    esz = {'bf16': 2, 'f32': 4, 'f64': 8}[dtype]
    msz = 8 if dtype == 'f64' else 4
    if form == 'entries':
        data, handed = ke, ke.known * (4 + msz) + (n_r + 1) * 8 + (n_r + n_c) * msz
    else:
        data, handed = dense_on_device(ke, dtype), n_r * n_c * esz
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
        out = dict(form=form, dtype=dtype, fill=fill, shape=[n_r, n_c], entries=ke.known, ranks=[c_r, c_c],
                   create_upload_bind_s=round(t1 - t0, 3), it_per_s=round(float(np.median(rates)), 2),
                   it_per_s_min=round(min(rates), 2), it_per_s_max=round(max(rates), 2),
                   workspace_bytes=plan.workspace_bytes, relation_device_bytes=handed,
                   host_peak_rss_bytes=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024, sqerr=err)
    finally:
        plan.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--dtypes', default='bf16,f32')
    ap.add_argument('--fills', default='mean,row_mean')
    ap.add_argument('--shape', default='100000,40000,800,128,256', help='n_row,n_col,per_row,rank_row,rank_col')
    ap.add_argument('--one', nargs=8, metavar=('FORM', 'DTYPE', 'FILL', 'N_ROW', 'N_COL', 'PER_ROW', 'RANK_ROW', 'RANK_COL'))
    a = ap.parse_args()
    if a.one:
        one(a.one[0], a.one[1], a.one[2], *[int(v) for v in a.one[3:]], iters=a.iters)
        return
    shape = a.shape.split(',')
    jobs = [(form, dtype, fill) for dtype in a.dtypes.split(',') for fill in a.fills.split(',') for form in ('entries', 'dense')]
    lines = []
    for form, dtype, fill in jobs:                       # every measurement: its own process, its own time limit
        cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--iters', str(a.iters), '--one',
               form, dtype, fill] + shape
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
