"""The k best columns of every row for any k (`_complete.DeviceCompleter.row_kth` / `row_best`, csrc/skf_complete.h
complete_row_digits_kernel / complete_row_walk_kernel) on one resident block of 8192 rows against 400 000 columns with 40
excluded columns per row, for BOTH widths of the select's digit (SKF_ROW_DIGIT_BITS = 8: 4 / 8 passes, one workgroup per CU;
7: 5 / 10 passes, two to three):

    python tools/bench_row_best.py [--out profiles/row_best.txt] [--configs 16:f32,128:f32,16:f64,128:f64] [--ks 100,1000]

The library is compiled once more with -DSKF_ROW_DIGIT_BITS=<the other width> (lib/libskfusion_hip_rowdigits<w>.so, built on
first use, `--build-only` to do nothing else) and each (configuration, width) runs in a child process of its own that loads one
of the two, under a time limit (--limit seconds); the first that fails or runs out of time ends the run.  Per configuration the
order is default width, other width, default width again: the two default lines are the spread of the box at that moment, and
within every child the yardsticks are timed before AND after the selects (an idle-box check: a drift between the two, or
between the two default lines, larger than the difference of the widths means the box was not idle).

One JSON line per (configuration, width), all times in ms, host clock around device-synchronised calls on resident operands,
median of --runs after a warm-up:
  row_kth_ms[k]      skf_complete_row_kth alone: list check, every counting pass and walk of the select
  per_pass_ms[k]     row_kth_ms / passes
  topk64_ms          the yardstick of ONE walk with a selection epilogue: skf_complete_topk, k = 64, same operands
  above_count_ms     the yardstick of ONE walk with a popcount epilogue: the count pass of skf_complete_above at the select's
                     thresholds (device pointer) -- [before, after] the selects
  row_best_ms[k]     DeviceCompleter.row_best whole: uploads, H = G S, select, count, fill, results back
Anything that did not run is not measured, and the record says so."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_ranks import chosen_splits, median_of, strided        # noqa: E402

BLOCK = 8192
PKG = os.path.join(ROOT, 'scikit-fusion_amd')


def default_bits():
    with open(os.path.join(PKG, 'csrc', 'skf_complete.h')) as fh:
        return int(re.search(r'#define SKF_ROW_DIGIT_BITS (\d+)', fh.read()).group(1))


def variant_library(bits, rebuild=False):
    """The library with the other digit width: skf_api.hip compiled once more, linked with the instantiation units of the
    product build.  None for the default width (the product library itself)."""
    if bits == default_bits():
        return None
    out = os.path.join(PKG, 'lib', 'libskfusion_hip_rowdigits%d.so' % bits)
    if os.path.exists(out) and not rebuild:
        return out
    import __graft_entry__
    __graft_entry__.build()
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    objdir = os.path.join(PKG, 'lib', 'obj')
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I', os.path.join(ROOT, 'include'), '-DSKF_SPLIT_BUILD']
    units = sorted(f for f in os.listdir(os.path.join(PKG, 'csrc')) if f.startswith('skf_inst_') and f.endswith('.hip'))
    objs = []
    for u in units:                                      # (left by the product build; compiled here only where they are missing)
        obj = os.path.join(objdir, u + '.o')
        if not os.path.exists(obj):
            subprocess.check_call([hipcc] + flags + ['-c', os.path.join(PKG, 'csrc', u), '-o', obj])
        objs.append(obj)
    api = os.path.join(objdir, 'skf_api.hip.rowdigits%d.o' % bits)
    subprocess.check_call([hipcc] + flags + ['-DSKF_ROW_DIGIT_BITS=%d' % bits, '-c', os.path.join(PKG, 'csrc', 'skf_api.hip'), '-o', api])
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-Wl,-z,defs', api] + objs + ['-o', out])
    return out


def run(c, dtype, bits, n_j, per_row, ks, runs):
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DeviceCompleter
    rt = nat.get_runtime()                               # (SKF_LIB_PATH names the library of this width)
    mem = rt.mem
    rs = np.random.RandomState(0)
    G_row = rs.rand(BLOCK, c) * 0.1 + 0.01
    S = rs.rand(c, c) * 0.2
    G_col = rs.rand(n_j, c) * 0.1 + 0.01
    excl = strided(rs, BLOCK, n_j, per_row)
    xl = (np.arange(BLOCK + 1, dtype=np.int64) * per_row, excl.reshape(-1))
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    code, m, es = comp.code, BLOCK, comp.es
    bh = mem.from_host(np.dot(G_row, S).astype(comp.npd))
    xp, xi = [mem.from_host(x) for x in xl]
    need = [C.c_size_t() for _ in range(3)]
    rt.call('skf_complete_row_kth_workspace_bytes', code, m, n_j, 0, C.byref(need[0]))
    rt.call('skf_complete_above_workspace_bytes', code, m, n_j, 0, C.byref(need[1]))
    rt.call('skf_complete_topk_workspace_bytes', code, m, n_j, 64, 0, C.byref(need[2]))
    ws = mem.empty(max(n.value for n in need))
    thr, greater, equal, cands = mem.empty(m * es), mem.empty(m * 8), mem.empty(m * 8), mem.empty(m * 8)
    op, oi, ov = mem.empty((m + 1) * 8), mem.empty(m * 64 * 4), mem.empty(m * 64 * es)
    nf = C.c_int64(0)

    def row_kth(k):
        want = mem.from_host(np.full(m, k, dtype=np.int64))

        def call():
            rt.call('skf_complete_row_kth', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, want.ptr, xp.ptr, xi.ptr, thr.ptr, greater.ptr,
                    equal.ptr, cands.ptr, 0, ws.ptr, ws.nbytes, mem.stream)
            mem.synchronize()
        return call

    def count_only():
        rt.call('skf_complete_above', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, thr.ptr, xp.ptr, xi.ptr, 0, op.ptr, None, None,
                C.byref(nf), 0, ws.ptr, ws.nbytes, mem.stream)
        mem.synchronize()

    def topk64():
        rt.call('skf_complete_topk', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, 64, xp.ptr, xi.ptr, oi.ptr, 64, ov.ptr, 64, 0,
                ws.ptr, ws.nbytes, mem.stream)
        mem.synchronize()

    passes = -(-8 * es // bits)
    row_kth(ks[0])()                                     # the thresholds the first count pass reads; code objects
    t_count0, _ = median_of(count_only, runs, 1)
    t_topk0, _ = median_of(topk64, runs, 1)
    t_kth, t_best, entries = {}, {}, {}
    for k in ks:
        t_kth[k], _ = median_of(row_kth(k), runs, 1)
        g = mem.to_host(greater, (m,), np.int64)
        e = mem.to_host(equal, (m,), np.int64)
        assert ((g < k) & (k <= g + e)).all() and (mem.to_host(cands, (m,), np.int64) == n_j - per_row).all()
        count_only()
        assert nf.value == int((g + e).sum()), 'P4: above holds %d entries, the select said %d' % (nf.value, (g + e).sum())
        entries[k] = nf.value
    t_count1, _ = median_of(count_only, runs, 1)
    t_topk1, _ = median_of(topk64, runs, 1)
    for k in ks:
        t_best[k], _ = median_of(lambda: comp.row_best(G_row, k, exclude=xl), runs, 1)
    ms = lambda t: round(1e3 * t, 3)                     # noqa: E731
    return dict(dtype=dtype, shape=[m, n_j], ranks=[c, c], excluded_per_row=per_row, digit_bits=bits, passes=passes,
                row_kth_ms={k: ms(t_kth[k]) for k in ks}, per_pass_ms={k: ms(t_kth[k] / passes) for k in ks},
                topk64_ms=[ms(t_topk0), ms(t_topk1)], above_count_ms=[ms(t_count0), ms(t_count1)],
                row_kth_to_count={k: round(2 * t_kth[k] / (t_count0 + t_count1), 2) for k in ks},
                row_best_ms={k: ms(t_best[k]) for k in ks}, entries=entries, col_splits_block_8192=chosen_splits(rt, code, m, n_j),
                device_peak_MiB=round(comp.peak_bytes / 2.0 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--configs', default='16:f32,128:f32,16:f64,128:f64', help='rank:dtype, comma separated')
    ap.add_argument('--ks', default='100,1000')
    ap.add_argument('--cols', type=int, default=400000)
    ap.add_argument('--excluded', type=int, default=40)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--limit', type=int, default=240, help='seconds a (configuration, width) may take')
    ap.add_argument('--build-only', action='store_true')
    ap.add_argument('--rebuild', action='store_true')
    ap.add_argument('--one', default=None, help='(internal) rank:dtype:bits -- run this one in this process')
    a = ap.parse_args()
    ks = [int(v) for v in a.ks.split(',')]
    if a.one:
        f = a.one.split(':')
        print(json.dumps(run(int(f[0]), f[1], int(f[2]), a.cols, a.excluded, ks, a.runs)), flush=True)
        return 0
    base = default_bits()
    other = 7 if base == 8 else 8
    libs = {base: None, other: variant_library(other, a.rebuild)}
    if a.build_only:
        print(libs[other])
        return 0

    def note(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')
    for cfg in a.configs.split(','):
        for bits in (base, other, base):
            env = dict(os.environ)
            if libs[bits]:
                env['SKF_LIB_PATH'] = libs[bits]
            cmd = [sys.executable, os.path.abspath(__file__), '--one', '%s:%d' % (cfg, bits), '--ks', a.ks, '--cols', str(a.cols),
                   '--excluded', str(a.excluded), '--runs', str(a.runs)]
            try:
                out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit, env=env)
            except subprocess.TimeoutExpired:
                note('configuration %s width %d ran past %d s: stopping; the rest is not measured' % (cfg, bits, a.limit))
                return 1
            if out.returncode != 0:
                note('configuration %s width %d failed (status %d): stopping; the rest is not measured' % (cfg, bits, out.returncode))
                return 1
            note(out.stdout.decode().strip().splitlines()[-1])
    return 0


if __name__ == '__main__':
    sys.exit(main())
