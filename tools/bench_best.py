"""The n best pairs of a whole relation (`FusionFit.complete_best`, `_complete.DeviceCompleter.kth` / `digits`,
csrc/skf_complete.h complete_digits_kernel) at 100 000 x 400 000 with 40 excluded columns per row, in blocks of 8192 rows:

    python tools/bench_best.py [--out profiles/best_pairs.txt] [--configs 16:f32,128:f32,128:f64:24576] [--n 100000]

Every configuration `rank:dtype[:rows]` runs in a child process of its own under a time limit (--limit seconds); the first
one that fails or runs out of time ends the run.  Per configuration one JSON line:
  digit_pass_s     one counting pass (`digits`, 11 key bits, empty prefix) over all blocks, whole call path: uploads of the
                   rows and their lists, H = G S, the list check, the launch; and the LAST pass of the selection (its full prefix)
  count_pass_s     the yardstick: the count-only pass of `above` at the selected threshold over the same blocks -- the parent
                   operator's kernel, the same tile product with a popcount epilogue
  kth_s, best_s    the whole `complete_kth` and the whole `complete_best` (n pairs, ties='first') through the public API
  kernel_*_ms      skf_complete_digits (first and last pass) and the count-only skf_complete_above alone on one resident block
                   of 8192 rows, device-synchronised, median of 5 after a warm-up; digits_to_count = their ratio: what the
                   histogram epilogue costs over the popcount epilogue, the only difference between the two kernels."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_ranks import chosen_splits, median_of, strided        # noqa: E402

BLOCK = 8192


def run(c, dtype, rows, n_i, n_j, per_row, n):
    import scipy.sparse
    import __graft_entry__
    __graft_entry__.build()
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DeviceCompleter
    from skfusion_amd.fusion import FusionGraph, ObjectType, Relation
    from skfusion_amd.fusion.base import FusionFit
    rt = nat.get_runtime()
    mem = rt.mem
    rs = np.random.RandomState(0)
    rows = min(rows or n_i, n_i)
    G_row = rs.rand(n_i, c)[:rows] * 0.1 + 0.01
    S = rs.rand(c, c) * 0.2
    G_col = rs.rand(n_j, c) * 0.1 + 0.01
    excl = strided(rs, n_i, n_j, per_row)[:rows]
    xs = scipy.sparse.csr_matrix((np.ones(excl.size, dtype=np.int8), excl.reshape(-1), np.arange(rows + 1, dtype=np.int64) * per_row),
                                 shape=(rows, n_j))
    a, b = ObjectType('rows', c), ObjectType('cols', c)
    rel = Relation(scipy.sparse.csr_matrix((rows, n_j)), a, b)
    fit = FusionFit()
    fit.fusion_graph, fit.n_run = FusionGraph([rel]), 1
    fit.factors_[a], fit.factors_[b], fit.backbones_[rel] = [G_row], [G_col], [S]

    def lists(r0, r1):
        return np.arange(r1 - r0 + 1, dtype=np.int64) * per_row, excl[r0:r1].reshape(-1)

    def blocks():
        for r0 in range(0, rows, BLOCK):
            r1 = min(r0 + BLOCK, rows)
            yield G_row[r0:r1], lists(r0, r1)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    comp = DeviceCompleter(S, G_col, dtype=dtype)
    comp.above(G_row[:BLOCK], np.inf, exclude=lists(0, min(BLOCK, rows)), count_only=True)      # warm-up: code objects, scratch
    t_kth, (T, g, e) = timed(lambda: fit.complete_kth(rel, n, exclude=xs, dtype=dtype, block_rows=BLOCK))
    t_best, best = timed(lambda: fit.complete_best(rel, n, exclude=xs, dtype=dtype, block_rows=BLOCK))
    assert best.nnz == n and best.data.min() == T

    plan = comp.DIGIT_PLAN[comp.es]
    bits = 8 * comp.es
    last_db = plan[-1]
    key = int(np.array([T], dtype=comp.npd).view('u%d' % comp.es)[0])
    key = key ^ ((1 << bits) - 1 if key >> (bits - 1) else 1 << (bits - 1))
    last_prefix = key >> last_db

    def digit_pass(prefix, pbits, db):
        hist = mem.from_host(np.zeros(1 << db, dtype=np.uint64))
        for A, xl in blocks():
            comp.digits(A, prefix, pbits, db, hist, exclude=xl)
        return mem.to_host(hist, (1 << db,), np.uint64)

    def count_pass():
        return sum(int(comp.above(A, T, exclude=xl, count_only=True)[-1]) for A, xl in blocks())
    t_first, h = timed(lambda: digit_pass(0, 0, plan[0]))
    t_last, _ = timed(lambda: digit_pass(last_prefix, bits - last_db, last_db))
    t_count, found = timed(count_pass)
    assert found == g + e and int(h.astype(object).sum()) == rows * (n_j - per_row)

    # the two kernels alone on one resident block
    code, m = comp.code, min(BLOCK, rows)
    bh = mem.from_host(np.dot(G_row[:m], S).astype(comp.npd))
    xp, xi = [mem.from_host(x) for x in lists(0, m)]
    need = C.c_size_t()
    rt.call('skf_complete_above_workspace_bytes', code, m, n_j, 0, C.byref(need))
    ws, op = mem.empty(need.value), mem.empty((m + 1) * 8)
    bt = mem.from_host(np.full(m, T, dtype=comp.npd))
    hist = mem.from_host(np.zeros(2048, dtype=np.uint64))
    nf = C.c_int64(0)

    def count_only():
        rt.call('skf_complete_above', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, bt.ptr, xp.ptr, xi.ptr, 0, op.ptr, None, None,
                C.byref(nf), 0, ws.ptr, ws.nbytes, mem.stream)
        mem.synchronize()

    def digits(prefix, pbits, db):
        def call():
            rt.call('skf_complete_digits', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, xp.ptr, xi.ptr, prefix, pbits, db, hist.ptr, 0,
                    ws.ptr, ws.nbytes, mem.stream)
            mem.synchronize()
        return call
    k_count, _ = median_of(count_only, 5, 1)
    k_first, _ = median_of(digits(0, 0, plan[0]), 5, 1)
    k_last, _ = median_of(digits(last_prefix, bits - last_db, last_db), 5, 1)
    k_count2, _ = median_of(count_only, 5, 1)                                # (once more: the drift of the clock across the three)
    return dict(dtype=dtype, shape=[rows, n_j], ranks=[c, c], excluded_per_row=per_row, n=n, block_rows=BLOCK, passes=len(plan),
                threshold=float(T), n_greater=g, n_equal=e, digit_pass_s=round(t_first, 3), last_digit_pass_s=round(t_last, 3),
                count_pass_s=round(t_count, 3), pass_ratio=round(t_first / t_count, 3), kth_s=round(t_kth, 3), best_s=round(t_best, 3),
                kernel_count_only_ms=[round(1e3 * k_count, 3), round(1e3 * k_count2, 3)], kernel_digits_first_ms=round(1e3 * k_first, 3),
                kernel_digits_last_ms=round(1e3 * k_last, 3), digits_to_count=round(2 * k_first / (k_count + k_count2), 3),
                last_digits_to_count=round(2 * k_last / (k_count + k_count2), 3), col_splits_block_8192=chosen_splits(rt, code, m, n_j),
                device_peak_MiB=round(comp.peak_bytes / 2.0 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--configs', default='16:f32,128:f32,128:f64:24576', help='rank:dtype[:rows timed], comma separated')
    ap.add_argument('--shape', default='100000,400000,40', help='n_i,n_j,excluded per row')
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--limit', type=int, default=240, help='seconds a configuration may take')
    ap.add_argument('--one', default=None, help='(internal) run this configuration in this process')
    a = ap.parse_args()
    n_i, n_j, per_row = [int(v) for v in a.shape.split(',')]
    if a.one:
        f = a.one.split(':')
        print(json.dumps(run(int(f[0]), f[1], int(f[2]) if len(f) > 2 else 0, n_i, n_j, per_row, a.n)), flush=True)
        return 0
    for cfg in a.configs.split(','):
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', cfg, '--shape', a.shape, '--n', str(a.n)],
                                 stdout=subprocess.PIPE, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print('configuration %s ran past %d s: stopping' % (cfg, a.limit), flush=True)
            return 1
        if out.returncode != 0:
            print('configuration %s failed (status %d): stopping' % (cfg, out.returncode), flush=True)
            return 1
        line = out.stdout.decode().strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
