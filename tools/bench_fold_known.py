"""Time of a fold-in on the KNOWN entries only (SKF_REL_FOLD_CSR | SKF_REL_FOLD_KNOWN, fusion.DfmcTransform): one iteration
of the plan (X = G B_r, one pass of fold_known_kernel over the lists, the side products, the update) and the pass alone
(skf_fold_known_pass on the same lists, with the bytes of the rows it gathers per second), beside the only alternative
before this form existed: the fold-in of DfmfTransform on the EXPANDED relation with its unknown cells filled with the mean
of the known ones (one dense n_new x n_partner matrix in the engine's type), per iteration and its preparation.

    python tools/bench_fold_known.py [--out profiles/fold_known.txt] [--deviations FILE]      the whole record
    python tools/bench_fold_known.py --one FORM DTYPE N_T N_P RANK_T RANK_P PER_ROW           one measurement (JSON line)
    python tools/bench_fold_known.py --planted                                           held-out RMSE of both fold-ins (JSON lines)

The record: 20 000 new users x 40 000 movies with 2 % known (800 per user, 16 M entries) at ranks 256 / 128 in f32 and bf16
plans, known-entry and expanded; 200 000 x 400 000 with 40 entries each at ranks 128 / 64 (bf16 plan; no expanded form:
320 GB); the held-out RMSE of DfmcTransform and of DfmfTransform (zero fill, mean fill) on planted data (120 x 300, ranks
8 / 6, noise 0.01, 10 % and 30 % known, f64, 100 iterations); and the f32 / bf16 deviations the GPU tests measured
(--deviations FILE: the table of measured deviations the test session writes at its end, tests/conftest.py).  Every measurement is a process of its own under its own `timeout
-k 10`; the first one that fails ends the run, and what was not measured is listed as not measured.  Times are medians of 7
device-synchronised runs after a warm-up."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def median_ms(fn, sync, n=8):
    times = []
    for _ in range(n):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(times[1:])), 3)


def one(form, dtype, n_t, n_p, c_t, c_p, per_row):
    import __graft_entry__
    __graft_entry__.build()
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DevicePlan, KnownEntries
    from bench_sparse_dfmf import entries
    rs = np.random.RandomState(1)
    Gp = rs.rand(n_p, c_p) * 0.1 + 0.01
    G0 = rs.rand(n_t, c_t) * 0.1 + 0.01
    S = (rs.rand(c_t, c_p) * 0.2).astype(np.float32)
    ke = entries(n_t, n_p, per_row)
    out = dict(form=form, dtype=dtype, shape=[n_t, n_p], entries=n_t * per_row, ranks=[c_t, c_p])
    if form == 'known':
        data = KnownEntries(ke.indptr, ke.indices, ke.values, ke.shape, unstored='unknown')
    else:                                   # DfmfTransform's view: expanded, the unknown cells hold the mean of the known ones
        import torch
        from skfusion_amd._engine import device_matrix_from_tensor
        tdt = {'bf16': torch.bfloat16, 'f32': torch.float32, 'f64': torch.float64}[dtype]
        R = torch.full(ke.shape, float(ke.values.mean()), dtype=tdt, device='cuda')
        R[torch.from_numpy(ke.row_of_entries()).cuda(), torch.from_numpy(ke.indices.astype(np.int64)).cuda()] = \
            torch.from_numpy(ke.values).cuda().to(tdt)
        torch.cuda.synchronize()
        data = device_matrix_from_tensor(R)
        out['relation_bytes'] = R.numel() * R.element_size()
    plan = DevicePlan(['new', 'old'], {'new': n_t, 'old': n_p}, {'new': c_t, 'old': c_p}, [('new', 'old', data, None)], [],
                      nat.SKF_TRANSFORM, dtype=dtype, target='new')
    try:
        plan.set_factor('old', Gp)
        plan.set_factor('new', G0)

        def prepare():
            plan.set_backbone(0, S)          # (marks the plan unprepared)
            plan.synchronize()
            t0 = time.perf_counter()
            plan.iterate(0)
            plan.synchronize()
            return time.perf_counter() - t0
        out['prepare_ms'] = round(1e3 * float(np.median([prepare() for _ in range(6)][1:])), 3)
        out['iteration_ms'] = round(median_ms(lambda: plan.iterate(5), plan.synchronize) / 5.0, 3)
        errs = [plan.relation_sqerr(0) for _ in range(1)]
        out['finite'] = bool(np.isfinite(plan.get_factor('new')).all() and np.isfinite(errs).all())
        out['workspace_bytes'] = plan.workspace_bytes
    finally:
        plan.close()
    if form == 'known':                     # the pass alone, on buffers of its own (masters: f32 in the bf16 plan)
        rt = nat.get_runtime()
        code = nat.SKF_F64 if dtype == 'f64' else nat.SKF_F32
        T_ = nat.NP_DTYPE[code]
        bufs = [rt.mem.from_host(a) for a in (ke.indptr, ke.indices, ke.values.astype(T_), G0.astype(T_),
                                              (Gp @ S.T.astype(np.float64)).astype(T_), np.zeros((n_t, c_t), T_),
                                              np.zeros((n_t, c_t), T_), np.zeros((n_t, c_t), T_))]
        bp, bi, bv, bg, bt, bx, be, bd = [b.ptr for b in bufs]
        run = lambda: rt.call('skf_fold_known_pass', code, bp, bi, bv, n_t, bg, c_t, bt, c_t, c_t, bx, c_t, be, c_t, bd, c_t, rt.mem.stream)
        out['pass_ms'] = median_ms(run, rt.mem.synchronize)
        out['pass_gathered_TB_per_s'] = round(n_t * per_row * c_t * np.dtype(T_).itemsize / (out['pass_ms'] * 1e-3) / 1e12, 3)
    print(json.dumps(out), flush=True)


def planted():
    """Held-out RMSE on planted data with the true partner factor and backbone frozen (tests/fold_known_cases.py states the
    same case as an assertion)."""
    import __graft_entry__
    __graft_entry__.build()
    from skfusion_amd.fusion.decomposition import _dfmf
    from skfusion_amd._engine import KnownEntries
    for share in (0.1, 0.3):
        rs = np.random.RandomState(0)
        nt, n_p, ct, cp = 120, 300, 8, 6
        Gp, Gt, S = rs.rand(n_p, cp), rs.rand(nt, ct), rs.rand(ct, cp)
        R = Gt @ S @ Gp.T + 0.01 * rs.randn(nt, n_p)
        pat = rs.rand(nt, n_p) < share
        pat[7] = False
        G0 = np.random.RandomState(1).rand(nt, ct)
        indptr = np.zeros(nt + 1, dtype=np.int64)
        np.cumsum(pat.sum(axis=1), out=indptr[1:])
        ke = KnownEntries(indptr, np.nonzero(pat)[1], R[pat], R.shape, unstored='unknown')
        fold = lambda data: _dfmf.transform({('new', 'old'): [data]}, {}, 'new', {'new': ct, 'old': cp}, {('old', 'old'): Gp},
                                            {('new', 'old'): [S]}, max_iter=100, dtype='f64', G0=G0)
        rmse = lambda G: round(float(np.sqrt((((R - G @ S @ Gp.T) ** 2)[~pat]).mean())), 4)
        print(json.dumps(dict(planted=True, known_share=share, rmse_known_entries=rmse(fold(ke)),
                              rmse_zero_fill=rmse(fold(np.where(pat, R, 0.0))),
                              rmse_mean_fill=rmse(fold(np.where(pat, R, R[pat].mean()))))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', nargs=7, metavar=('FORM', 'DTYPE', 'N_T', 'N_P', 'RANK_T', 'RANK_P', 'PER_ROW'))
    ap.add_argument('--planted', action='store_true')
    ap.add_argument('--deviations', default=None, metavar='FILE',
                    help='the deviations table a GPU run of the test suite wrote (tests/conftest.py, pytest_sessionfinish)')
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], a.one[1], *[int(v) for v in a.one[2:]])
    if a.planted:
        return planted()
    me = os.path.abspath(__file__)
    jobs = [(['--planted'], 300)]
    for dt in ('f32', 'bf16'):
        jobs.append((['--one', 'known', dt, '20000', '40000', '256', '128', '800'], 300))
        jobs.append((['--one', 'expanded', dt, '20000', '40000', '256', '128', '800'], 300))
    jobs.append((['--one', 'known', 'bf16', '200000', '400000', '128', '64', '40'], 300))
    lines, ok = [], True
    for n, (args, limit) in enumerate(jobs):                # every measurement: its own process, its own time limit
        done = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, me] + args, stdout=subprocess.PIPE, universal_newlines=True)
        got = [l for l in done.stdout.splitlines() if l.startswith('{')]
        for l in got:
            print(l, flush=True)
        lines += got
        if done.returncode != 0:
            missed = ['%s: ended with status %d -- not measured; stopping here' % (' '.join(args), done.returncode)]
            missed += ['%s: not measured' % ' '.join(rest) for rest, _ in jobs[n + 1:]]
            print('\n'.join(missed), flush=True)
            lines += missed
            ok = False
            break
    found = []
    if a.deviations and os.path.exists(a.deviations):
        with open(a.deviations) as fh:
            found = [l.rstrip() for l in fh if l.startswith('GPU') and 'known-entry fold-in vs its f64' in l]
    lines.append('deviations of the GPU tests (check / measured / bound = 4 x the zero-filled dense-fed plan\'s / bound : measured):')
    lines += found or ['not measured (no --deviations table of a GPU run of the suite was given)']
    if a.out:
        with open(a.out, 'a') as fh:
            for l in lines:
                fh.write(l + '\n')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
