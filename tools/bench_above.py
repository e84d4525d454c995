"""Scores at or above a per-row threshold as CSR at BASELINE config 5's shape -- 100 000 users x 40 000 movies, ranks
256 / 256, 80 M excluded (known) pairs -- selected on the device (`_complete.DeviceCompleter.above`, csrc/skf_complete.h) against

  (a) the only route the project had before: `DeviceReconstructor.block` (what `complete_blocks(block_rows=4096)` runs per
      block) pulled to the host, the known pairs masked, one `>=` and one `nonzero` per block, in the same process;
  (b) `DeviceCompleter.topk` with k = 64 on the same blocks: one pass over the same tiles, the scale of the matrix work.

    python tools/bench_above.py [--out profiles/r20_above.txt] [--dtypes f32,f64] [--blocks 2] [--rounds 3]

The thresholds are per row the 64th, the 400th and the 4000th score, estimated on the host from the row's float64 scores on a
fixed sample of 4000 columns (their 6th, 40th and 400th).  Per dtype and threshold one JSON line:
  above     whole call path of `DeviceCompleter.above` over the first --blocks blocks of 8192 rows (uploads of the rows and
            their lists, H = G S, the list check, count, scan, fill, results back), seconds per block: median, min, max of
            --rounds runs that ALTERNATE with the other two routes; entries per row found;
  host      (a) on as many rows in blocks of 4096, seconds per 8192 rows; topk64: (b) likewise;
  kernel    skf_complete_above alone on one resident block of 8192 rows, device-synchronised, median of 5 after a warm-up:
            count only (out_indices NULL) and the full call with sufficient capacity -- the difference is what the second walk
            over the tiles and the stores cost; skf_complete_topk (k = 64) on that block beside them."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_ranks import chosen_splits, median_of, strided        # noqa: E402

NTH = (64, 400, 4000)
SAMPLE = 4000


def stats(times, scale=1.0):
    return dict(median=round(float(np.median(times)) * scale, 4), min=round(min(times) * scale, 4), max=round(max(times) * scale, 4))


def run(dtype, n_i, n_j, c, per_row, blocks, rounds, emit):
    import __graft_entry__
    __graft_entry__.build()
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DeviceCompleter, DeviceReconstructor
    rt = nat.get_runtime()
    mem = rt.mem
    rs = np.random.RandomState(0)
    block = 8192
    rows = min(n_i, blocks * block)
    G_row = rs.rand(n_i, c)[:rows] * 0.1 + 0.01
    S = rs.rand(c, c) * 0.2
    G_col = rs.rand(n_j, c) * 0.1 + 0.01
    excl = strided(rs, n_i, n_j, per_row)[:rows]
    comp = DeviceCompleter(S, G_col, dtype=dtype)
    rec = DeviceReconstructor(S, G_col, dtype=dtype)
    cols = np.sort(rs.choice(n_j, size=min(SAMPLE, n_j), replace=False))
    Xs = -np.sort(-np.dot(np.dot(G_row, S), G_col[cols].T), axis=1)          # the rows' sampled scores, best first

    def lists(r0, r1):
        return np.arange(r1 - r0 + 1, dtype=np.int64) * per_row, excl[r0:r1].reshape(-1)

    code, T = comp.code, comp.npd
    m = min(block, rows)
    bh = mem.from_host(np.dot(G_row[:m], S).astype(T))
    xp, xi = [mem.from_host(a) for a in lists(0, m)]
    need = C.c_size_t()
    rt.call('skf_complete_topk_workspace_bytes', code, m, n_j, 64, 0, C.byref(need))
    tws, toi, tov = mem.empty(need.value), mem.empty(m * 64 * 4), mem.empty(m * 64 * comp.es)

    def topk_alone():
        rt.call('skf_complete_topk', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, 64, xp.ptr, xi.ptr, toi.ptr, 64, tov.ptr, 64, 0,
                tws.ptr, tws.nbytes, mem.stream)
        mem.synchronize()
    comp.topk(G_row[:m], 64, exclude=lists(0, m))                            # warm-up: code objects, scratch
    rec.block(G_row[:4096])
    tb_topk, _ = median_of(topk_alone, 5, 1)

    for nth in NTH:
        thr = Xs[:, max(1, int(round(nth * len(cols) / float(n_j)))) - 1].astype(T)
        found = [0]

        def above_path():
            found[0] = 0
            for r0 in range(0, rows, block):
                r1 = min(r0 + block, rows)
                found[0] += int(comp.above(G_row[r0:r1], thr[r0:r1], exclude=lists(r0, r1))[0][-1])

        def host_path():
            n = 0
            for r0 in range(0, rows, 4096):
                r1 = min(r0 + 4096, rows)
                X = rec.block(G_row[r0:r1])
                X[np.repeat(np.arange(r1 - r0), per_row), excl[r0:r1].reshape(-1)] = -np.inf
                r, j = np.nonzero(X >= thr[r0:r1, None].astype(np.float64))
                n += X[r, j].size
            return n

        def topk_path():
            for r0 in range(0, rows, block):
                r1 = min(r0 + block, rows)
                comp.topk(G_row[r0:r1], 64, exclude=lists(r0, r1))

        above_path()                                                         # warm-up: the scratch grows to what this threshold needs
        t = {'above': [], 'host': [], 'topk64': []}
        for _ in range(rounds):
            for name, fn in (('above', above_path), ('host', host_path), ('topk64', topk_path)):
                t0 = time.perf_counter()
                fn()
                t[name].append(time.perf_counter() - t0)
        per_block = float(block) / rows

        # the operator alone on resident data
        bt = mem.from_host(thr[:m])
        rt.call('skf_complete_above_workspace_bytes', code, m, n_j, 0, C.byref(need))
        ws, op = mem.empty(need.value), mem.empty((m + 1) * 8)
        nf = C.c_int64(0)

        def count_only():
            rt.call('skf_complete_above', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, bt.ptr, xp.ptr, xi.ptr, 0, op.ptr, None, None,
                    C.byref(nf), 0, ws.ptr, ws.nbytes, mem.stream)
            mem.synchronize()
        count_only()
        cap = max(nf.value, 1)
        oi, ov = mem.empty(cap * 4), mem.empty(cap * comp.es)

        def full():
            rt.call('skf_complete_above', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, bt.ptr, xp.ptr, xi.ptr, cap, op.ptr, oi.ptr, ov.ptr,
                    C.byref(nf), 0, ws.ptr, ws.nbytes, mem.stream)
            mem.synchronize()
        tb_count, _ = median_of(count_only, 5, 1)
        tb_full, full_all = median_of(full, 5, 1)
        del oi, ov
        emit(dict(dtype=dtype, shape=[n_i, n_j], ranks=[c, c], nth_score=nth, rows_timed=rows, excluded_per_row=per_row,
                  entries_per_row=round(found[0] / float(rows), 1),
                  above_s_per_block=stats(t['above'], per_block), host_s_per_block=stats(t['host'], per_block),
                  topk64_s_per_block=stats(t['topk64'], per_block),
                  speedup_over_host=round(float(np.median(t['host'])) / float(np.median(t['above'])), 1),
                  kernel_count_only_ms=round(1e3 * tb_count, 3), kernel_full_ms=round(1e3 * tb_full, 3),
                  kernel_full_ms_min=round(1e3 * min(full_all), 3), kernel_full_ms_max=round(1e3 * max(full_all), 3),
                  kernel_entries=int(nf.value), topk64_block_ms=round(1e3 * tb_topk, 3),
                  kernel_full_ratio_to_topk64=round(tb_full / tb_topk, 3), col_splits_block_8192=chosen_splits(rt, code, m, n_j),
                  device_peak_MiB=round(comp.peak_bytes / 2.0 ** 20, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--dtypes', default='f32,f64')
    ap.add_argument('--shape', default='100000,40000,256,800', help='n_i,n_j,rank,excluded per row')
    ap.add_argument('--blocks', type=int, default=2, help='blocks of 8192 rows every route is timed on')
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    n_i, n_j, c, per_row = [int(v) for v in a.shape.split(',')]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')
    for dt in a.dtypes.split(','):
        run(dt, n_i, n_j, c, per_row, a.blocks, a.rounds, emit)


if __name__ == '__main__':
    main()
