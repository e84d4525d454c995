"""Time of the sparse constraint pass (theta_spmm_kernel, and the hub kernels where rows are split) per threshold
SKF_THETA_HUB_ROW, dense-fed and entries-fed, and the bind time / HBM footprint of both forms.

    python tools/bench_theta_csr.py --case hub --n 32768   --form dense   --hub 0,1024,4096,16384
    python tools/bench_theta_csr.py --case hub --n 1000000 --form entries --hub 0,1024,4096,16384
    python tools/bench_theta_csr.py --case c5  --form dense,entries       --hub 0,4096
    ... --hub none      leaves the environment alone (a library that has no such switch: the commit before the split)

The graph: one constrained type of n objects (rank 128, f32 engine) and a partner of 16 objects (rank 8) with one dense
relation, so that everything but the constraint pass is small.  `hub`: about 8 entries a row (-0.001, ascending strided
buckets) plus the diagonal 0.02 plus row 0 holding n / 2 entries of -1e-6.  `c5`: bench.py's config-5 constraints on 40 000
movies (lambda I and a symmetric similarity pattern of about 2 entries a row), no hub.

What is timed: the stage of the iteration that ends in the constraint pass (skf_stage, SKF_STAGE_ACCUMULATE; the side
updates of the one thin relation come before it in the same stage), between two hipEvents on the engine's stream, 5 repeats
after a warm-up; the same stage of the same graph WITHOUT the constraint is timed alongside, so that the pass alone is the
difference.  One JSON line per (form, threshold)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hub_entries(n, per=8):
    """(indptr, indices, values) of the hub constraint, canonical CSR."""
    rs = np.random.RandomState(0)
    width = n // per
    cols = rs.randint(0, width, (n, per)).astype(np.int64) + (np.arange(per, dtype=np.int64) * width)[None, :]
    own = np.arange(n, dtype=np.int64)[:, None]
    clash = cols == own
    cols[clash] += np.where(cols[clash] % width == width - 1, -1, 1)
    cols = np.concatenate([cols, own], axis=1)
    vals = np.concatenate([np.full((n, per), -0.001), np.full((n, 1), 0.02)], axis=1)
    order = np.argsort(cols, axis=1)
    cols, vals = np.take_along_axis(cols, order, axis=1), np.take_along_axis(vals, order, axis=1)
    hub_cols = np.concatenate([[0], np.arange(1, n, 2)])
    hub_vals = np.concatenate([[0.02], np.full(hub_cols.size - 1, -1e-6)])
    indices = np.concatenate([hub_cols, cols[1:].reshape(-1)]).astype(np.int32)
    values = np.concatenate([hub_vals, vals[1:].reshape(-1)])
    counts = np.full(n, per + 1, dtype=np.int64)
    counts[0] = hub_cols.size
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    return indptr, indices, values


def c5_entries(n):
    """config 5's two constraints: lambda I, and a symmetric pattern of about 2 entries a row, weight -0.001."""
    rs = np.random.RandomState(1)
    i, j = rs.randint(0, n, n), rs.randint(0, n, n)
    keep = i != j
    i, j = np.concatenate([i[keep], j[keep]]), np.concatenate([j[keep], i[keep]])
    import scipy.sparse
    sim = scipy.sparse.csr_matrix((np.ones(i.size), (i, j)), shape=(n, n))
    sim.sum_duplicates()
    sim.sort_indices()
    sim.data[:] = -0.001
    eye = (np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.full(n, 0.01))
    return [eye, (sim.indptr.astype(np.int64), sim.indices.astype(np.int32), sim.data)]


def as_form(lists, n, form, rt):
    """The constraint in the form the plan takes: KnownEntries, or a dense f32 matrix assembled on the device."""
    from skfusion_amd._engine import device_matrix_from_tensor
    indptr, indices, values = lists
    if form == 'entries':
        from skfusion_amd._engine import KnownEntries
        return KnownEntries(indptr, indices, values, (n, n), unstored='zero'), 0
    import torch
    dense = torch.zeros((n, n), dtype=torch.float32, device='cuda')
    rows = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))).cuda()
    dense[rows, torch.from_numpy(indices.astype(np.int64)).cuda()] = torch.from_numpy(values.astype(np.float32)).cuda()
    torch.cuda.synchronize()
    dm = device_matrix_from_tensor(dense)
    dm.nnz = int(indices.size)
    return dm, n * n * 4


def stage_times(plan, rt, repeats=5):
    """ms of SKF_STAGE_ACCUMULATE, `repeats` times after one whole staged iteration and one more warm-up of the stage."""
    import torch
    import skfusion_amd._native as nat
    for st in (nat.SKF_STAGE_CONTRACT, nat.SKF_STAGE_BACKBONE, nat.SKF_STAGE_ACCUMULATE, nat.SKF_STAGE_UPDATE,
               nat.SKF_STAGE_CONTRACT, nat.SKF_STAGE_BACKBONE, nat.SKF_STAGE_ACCUMULATE):
        plan.stage(st)
    plan.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with rt.mem.stream_scope():
            a.record()
        plan.stage(nat.SKF_STAGE_ACCUMULATE)
        with rt.mem.stream_scope():
            b.record()
        plan.synchronize()
        out.append(a.elapsed_time(b))
    return out


def run(case, n, forms, hubs, c=128):
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DevicePlan
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    rt = nat.get_runtime()
    rs = np.random.RandomState(2)
    types, nn, rank = ['obj', 'p'], {'obj': n, 'p': 16}, {'obj': c, 'p': 8}
    rels = [('obj', 'p', rs.rand(n, 16).astype(np.float32), None)]
    G0 = {'obj': (rs.rand(n, c) * 0.1 + 0.01).astype(np.float32), 'p': (rs.rand(16, 8) + 0.1).astype(np.float32)}
    lists = [hub_entries(n)] if case == 'hub' else c5_entries(n)
    longest = max(int(np.diff(l[0]).max()) for l in lists)

    def timed(thetas):
        t0 = time.perf_counter()
        plan = DevicePlan(types, nn, rank, rels, thetas, nat.SKF_DFMF, dtype='f32')
        plan.synchronize()
        bind_s = time.perf_counter() - t0
        try:
            for t in types:
                plan.set_factor(t, G0[t])
            return stage_times(plan, rt), bind_s, plan.workspace_bytes
        finally:
            plan.close()

    base, _, ws0 = timed([])
    for form in forms:
        for hub in hubs:
            if hub != 'none':
                os.environ['SKF_THETA_HUB_ROW'] = hub
            given = [as_form(l, n, form, rt) for l in lists]
            ms, bind_s, ws = timed([('obj', g[0]) for g in given])
            print(json.dumps(dict(case=case, n=n, rank=c, form=form, hub_row=hub, nnz=int(sum(l[1].size for l in lists)),
                                  longest_row=longest, stage_ms=[round(v, 4) for v in ms], stage_ms_median=round(float(np.median(ms)), 4),
                                  spread_ms=round(max(ms) - min(ms), 4), base_stage_ms_median=round(float(np.median(base)), 4),
                                  pass_ms=round(float(np.median(ms) - np.median(base)), 4), create_upload_bind_s=round(bind_s, 3),
                                  workspace_bytes=ws, workspace_growth_bytes=ws - ws0, caller_dense_bytes=int(sum(g[1] for g in given)))),
                  flush=True)
            del given


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='hub', choices=('hub', 'c5'))
    ap.add_argument('--n', type=int, default=0)
    ap.add_argument('--form', default='dense')
    ap.add_argument('--hub', default='0,1024,4096,16384')
    a = ap.parse_args()
    n = a.n or (40000 if a.case == 'c5' else 32768)
    run(a.case, n, a.form.split(','), a.hub.split(','))


if __name__ == '__main__':
    main()
