"""The histogram walk (`_complete.DeviceCompleter.hist`, csrc/skf_complete.h complete_hist_kernel) on one resident block of 8192
rows against 400 000 columns with 40 excluded columns per row, relative to the count pass of skf_complete_above at the same shape:

    python tools/bench_hist.py [--out profiles/histogram.txt] [--configs 16:f32,128:f32,16:f64,128:f64] [--edges 16,256,2047]

Each configuration runs in a child process of its own under a time limit (--limit seconds); the first that fails or runs out of
time ends the run.  Within every child the yardsticks are timed before AND after the histogram walks (an idle-box check: a drift
between the two larger than the differences read from the table means the box was not idle).

One JSON line per configuration, all times in ms, host clock around device-synchronised calls on resident operands, median of
--runs after a warm-up:
  hist_ms[n_edges]       skf_complete_hist alone, no targets: list and edge check, one walk
  hist_tgt_ms[n_edges]   ... with 8192 x 20 targets
  above_count_ms         the yardstick of ONE walk with a popcount epilogue: the count pass of skf_complete_above at the
                         median edge in every row -- [before, after] the walks
  digits11_ms            one pass of skf_complete_digits over the top 11 key bits: the walk that bins by key bits -- [before, after]
  hist_to_count[n]       hist_ms / the mean of the two count passes; hist_tgt_to_count likewise
The edges are evenly spaced quantiles of the float64 scores of the block's first 16 rows, so that the bins hold like numbers of
candidates; P6 is checked at the median edge in every child.  Anything that did not run is not measured, and the record says so."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_ranks import chosen_splits, median_of, strided        # noqa: E402

BLOCK = 8192


def run(c, dtype, n_j, per_row, per_tgt, edge_counts, runs):
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DeviceCompleter
    rt = nat.get_runtime()
    mem = rt.mem
    rs = np.random.RandomState(0)
    G_row = rs.rand(BLOCK, c) * 0.1 + 0.01
    S = rs.rand(c, c) * 0.2
    G_col = rs.rand(n_j, c) * 0.1 + 0.01
    excl = strided(rs, BLOCK, n_j, per_row)
    tgts = strided(rs, BLOCK, n_j, per_tgt)
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    code, m, es = comp.code, BLOCK, comp.es
    H = np.dot(G_row, S)
    bh = mem.from_host(H.astype(comp.npd))
    xp, xi = mem.from_host(np.arange(m + 1, dtype=np.int64) * per_row), mem.from_host(excl.reshape(-1))
    tp, ti = mem.from_host(np.arange(m + 1, dtype=np.int64) * per_tgt), mem.from_host(tgts.reshape(-1))
    need = [C.c_size_t() for _ in range(3)]
    rt.call('skf_complete_hist_workspace_bytes', code, m, n_j, m * per_tgt, 0, C.byref(need[0]))
    rt.call('skf_complete_above_workspace_bytes', code, m, n_j, 0, C.byref(need[1]))
    rt.call('skf_complete_digits_workspace_bytes', code, m, n_j, 0, C.byref(need[2]))
    ws = mem.empty(max(n.value for n in need))
    sample = np.dot(H[:16], G_col.T)
    op = mem.empty((m + 1) * 8)
    nf = C.c_int64(0)
    thr_value = float(np.quantile(sample, 0.5).astype(comp.npd))
    thr = mem.from_host(np.full(m, thr_value, dtype=comp.npd))
    dhist = mem.from_host(np.zeros(2048, dtype=np.uint64))

    def count_only():
        rt.call('skf_complete_above', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, thr.ptr, xp.ptr, xi.ptr, 0, op.ptr, None, None,
                C.byref(nf), 0, ws.ptr, ws.nbytes, mem.stream)
        mem.synchronize()

    def digits11():
        rt.call('skf_complete_digits', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, xp.ptr, xi.ptr, 0, 0, 11, dhist.ptr, 0, ws.ptr,
                ws.nbytes, mem.stream)
        mem.synchronize()

    def hist(edges, with_targets):
        e = mem.from_host(edges)
        h = mem.from_host(np.zeros(edges.size + 1, dtype=np.uint64))
        t = mem.from_host(np.zeros(edges.size + 1, dtype=np.uint64))

        def call():
            rt.call('skf_complete_hist', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, e.ptr, edges.size, xp.ptr, xi.ptr,
                    tp.ptr if with_targets else None, ti.ptr if with_targets else None, m * per_tgt if with_targets else 0, h.ptr,
                    t.ptr if with_targets else None, 0, ws.ptr, ws.nbytes, mem.stream)
            mem.synchronize()
        return call, h, t

    count_only()
    found = nf.value
    t_count0, _ = median_of(count_only, runs, 1)
    t_dig0, _ = median_of(digits11, runs, 1)
    t_hist, t_tgt = {}, {}
    for n in edge_counts:
        edges = np.quantile(sample, (np.arange(n) + 0.5) / n).astype(comp.npd)
        edges[n // 2] = thr_value                        # (the quantiles ascend and the median is one of them up to rounding)
        edges = np.sort(edges)
        for with_targets, out in ((False, t_hist), (True, t_tgt)):
            call, h, t = hist(edges, with_targets)
            out[n], _ = median_of(call, runs, 1)
            counts = mem.to_host(h, (n + 1,), np.uint64).astype(object) // (runs + 1)
            assert int(counts.sum()) == m * (n_j - per_row), 'not every candidate is counted once per call'
            at = int(np.searchsorted(edges, thr_value, side='left'))
            assert int(counts[at + 1:].sum()) == found, 'P6: %d at or above the median edge, above() finds %d' % (counts[at + 1:].sum(), found)
            if with_targets:
                assert 0 < int(mem.to_host(t, (n + 1,), np.uint64).astype(object).sum()) // (runs + 1) <= m * per_tgt
    t_count1, _ = median_of(count_only, runs, 1)
    t_dig1, _ = median_of(digits11, runs, 1)
    ms = lambda v: round(1e3 * v, 3)                     # noqa: E731
    mean = 0.5 * (t_count0 + t_count1)
    return dict(dtype=dtype, shape=[m, n_j], ranks=[c, c], excluded_per_row=per_row, targets_per_row=per_tgt,
                hist_ms={n: ms(t_hist[n]) for n in edge_counts}, hist_tgt_ms={n: ms(t_tgt[n]) for n in edge_counts},
                above_count_ms=[ms(t_count0), ms(t_count1)], digits11_ms=[ms(t_dig0), ms(t_dig1)],
                hist_to_count={n: round(t_hist[n] / mean, 2) for n in edge_counts},
                hist_tgt_to_count={n: round(t_tgt[n] / mean, 2) for n in edge_counts},
                col_splits_block_8192=chosen_splits(rt, code, m, n_j))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--configs', default='16:f32,128:f32,16:f64,128:f64', help='rank:dtype, comma separated')
    ap.add_argument('--edges', default='16,256,2047')
    ap.add_argument('--cols', type=int, default=400000)
    ap.add_argument('--excluded', type=int, default=40)
    ap.add_argument('--targets', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--limit', type=int, default=120, help='seconds a configuration may take')
    ap.add_argument('--one', default=None, help='(internal) rank:dtype -- run this one in this process')
    a = ap.parse_args()
    edge_counts = [int(v) for v in a.edges.split(',')]
    if a.one:
        f = a.one.split(':')
        print(json.dumps(run(int(f[0]), f[1], a.cols, a.excluded, a.targets, edge_counts, a.runs)), flush=True)
        return 0
    import __graft_entry__
    __graft_entry__.build()

    def note(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')
    for cfg in a.configs.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--one', cfg, '--edges', a.edges, '--cols', str(a.cols),
               '--excluded', str(a.excluded), '--targets', str(a.targets), '--runs', str(a.runs)]
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)
        except subprocess.TimeoutExpired:
            note('configuration %s ran past %d s: stopping; the rest is not measured' % (cfg, a.limit))
            return 1
        if out.returncode != 0:
            note('configuration %s failed (status %d): stopping; the rest is not measured' % (cfg, out.returncode))
            return 1
        note(out.stdout.decode().strip().splitlines()[-1])
    return 0


if __name__ == '__main__':
    sys.exit(main())
