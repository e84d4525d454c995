"""Preparation time of a fold-in (SKF_TRANSFORM) through a relation handed over as its stored entries, compressed along the
target's side (SKF_REL_FOLD_CSR: T = G_p S^T, one pass of fold_lists_kernel), against the SAME data handed over as a dense
matrix (the path a scipy.sparse relation took before: toarray(), P = R G_p on the matrix cores, then P S^T), per engine and
density -- the crossover behind DfmfTransform's default rule -- and the time of one target object whose list holds every
partner (400 000 entries: the list runs serially in its lanes).

    python tools/bench_sparse_foldin.py [--out profiles/r10_sparse_foldin.txt]            the whole table
    python tools/bench_sparse_foldin.py --one DTYPE N_T N_P RANK_T RANK_P PER_ROW[,PER_ROW..]   one engine (JSON lines)

The table: 100 000 new objects x 40 000 partners, ranks 128 / 128, densities 1e-3, 1e-2, 4/128 (the fit's rule
density * rank <= 4) and 1/16, list-fed and dense-fed, engines f64 / f32 / bf16; then 1 x 400 000 with every entry stored,
f32.  Every engine is a process of its own under its own `timeout -k 10`; the first one that fails ends the run.  The dense
form is assembled on the device.  Per measurement: the preparation alone (skf_iterate with 0 iterations after
skf_set_backbone: everything prepare_transform does, device-synchronised), median of 7 after a warm-up; plan creation +
upload + bind (s); workspace bytes."""
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


def one(dtype, n_t, n_p, c_t, c_p, per_rows):
    import __graft_entry__
    __graft_entry__.build()
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DevicePlan
    from bench_sparse_dfmf import entries, dense_on_device
    rs = np.random.RandomState(1)
    Gp = rs.rand(n_p, c_p) * 0.1 + 0.01
    G0 = rs.rand(n_t, c_t) * 0.1 + 0.01
    S = (rs.rand(c_t, c_p) - 0.3).astype(np.float32)
    for per_row in per_rows:
        ke = entries(n_t, n_p, per_row)
        forms = ('lists', 'dense') if n_t > 1 else ('lists',)
        for form in forms:
            data = ke if form == 'lists' else dense_on_device(ke, dtype)
            t0 = time.perf_counter()
            plan = DevicePlan(['new', 'old'], {'new': n_t, 'old': n_p}, {'new': c_t, 'old': c_p}, [('new', 'old', data, None)], [],
                              nat.SKF_TRANSFORM, dtype=dtype, target='new')
            plan.synchronize()
            t1 = time.perf_counter()
            try:
                plan.set_factor('old', Gp)
                plan.set_factor('new', G0)
                times = []
                for k in range(8):
                    plan.set_backbone(0, S)              # (marks the plan unprepared)
                    plan.synchronize()
                    t2 = time.perf_counter()
                    plan.iterate(0)                      # the preparation alone
                    plan.synchronize()
                    times.append(time.perf_counter() - t2)
                plan.iterate(2)
                finite = bool(np.isfinite(plan.get_factor('new')).all())
                out = dict(form=form, dtype=dtype, shape=[n_t, n_p], entries=n_t * per_row, density=per_row / float(n_p),
                           ranks=[c_t, c_p], prepare_ms=round(1e3 * float(np.median(times[1:])), 3),
                           prepare_ms_min=round(1e3 * min(times[1:]), 3), prepare_ms_max=round(1e3 * max(times[1:]), 3),
                           create_upload_bind_s=round(t1 - t0, 3), workspace_bytes=plan.workspace_bytes, finite=finite)
            finally:
                plan.close()
            del data
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--dtypes', default='bf16,f32,f64')
    ap.add_argument('--one', nargs=6, metavar=('DTYPE', 'N_T', 'N_P', 'RANK_T', 'RANK_P', 'PER_ROWS'))
    a = ap.parse_args()
    if a.one:
        one(a.one[0], *[int(v) for v in a.one[1:5]], per_rows=[int(v) for v in a.one[5].split(',')])
        return
    jobs = [(dt, 100000, 40000, 128, 128, '40,400,1250,2500', 420) for dt in a.dtypes.split(',')]
    jobs.append(('f32', 1, 400000, 128, 64, '400000', 300))
    lines, ok = [], True
    for dt, n_t, n_p, c_t, c_p, per, limit in jobs:      # every engine: its own process, its own time limit
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--one', dt, str(n_t), str(n_p),
               str(c_t), str(c_p), per]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        for l in done.stdout.splitlines():
            if l.startswith('{'):
                print(l, flush=True)
                lines.append(json.loads(l))
        if done.returncode != 0:
            print('measurement %r ended with status %d: stopping here' % (cmd[6:], done.returncode), flush=True)
            ok = False
            break
    if a.out:
        with open(a.out, 'a') as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + '\n')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
