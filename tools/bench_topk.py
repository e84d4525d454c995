"""Top-k completion at BASELINE config 5's shape -- 100 000 users x 40 000 movies, ranks 256 / 256, k = 10, 80 M excluded
(known) pairs -- fused on the device (`_complete.DeviceCompleter.topk`, csrc/skf_complete.h) against the only route the
project had before: `DeviceReconstructor.block` (what `complete_blocks(block_rows=4096)` runs per block) pulled to the host,
the known pairs masked, `np.argpartition` + a sort of the k per row.

    python tools/bench_topk.py [--out profiles/r11_topk.txt] [--dtypes f32,f64] [--host-blocks 2]

Per dtype, JSON lines:
  fused     whole call path over every row in blocks of 8192 (uploads of the row blocks and their exclusion lists, H = G S,
            the pass, the merge, results back), seconds, median of 3 after a warm-up pass over one block;
  kernel    skf_complete_topk alone on one resident block of 8192 rows with its lists, device-synchronised, median of 7
            after 2 warm-ups, scaled to all rows; frac = t_min / t_kernel by bench.py's convention with t_min = the score
            flops 2 m n c at the dtype's matrix peak (157.3 / 78.6 TFLOP/s) -- one read of G_col per 64-row tile comes from
            the caches and is not the binding term at rank 256;
  host      the previous route on the first --host-blocks blocks of 4096 rows, scaled to all rows (it moves 32 GB at full
            size; the scaling is stated in the record);
  splits    the col_splits the library chooses for m = 100 000 (per block of 8192) and for m = 64."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = {'f32': 157.3, 'f64': 78.6}        # bench.py: MI355X dense matrix peaks


def chosen_splits(rt, code, m, n_cols, k):
    """The count behind a col_splits = 0 query: the explicit count whose workspace is the same (1 when no partial lists)."""
    need, probe = C.c_size_t(), C.c_size_t()
    rt.call('skf_complete_topk_workspace_bytes', code, m, n_cols, k, 0, C.byref(need))
    for s in range(1, 33):
        rt.call('skf_complete_topk_workspace_bytes', code, m, n_cols, k, s, C.byref(probe))
        if probe.value == need.value:
            return s
    return None


def run(dtype, n_i, n_j, c, k, per_row, host_blocks):
    import __graft_entry__
    __graft_entry__.build()
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DeviceCompleter, DeviceReconstructor
    rt = nat.get_runtime()
    mem = rt.mem
    rs = np.random.RandomState(0)
    G_row = rs.rand(n_i, c) * 0.1 + 0.01
    S = rs.rand(c, c) * 0.2
    G_col = rs.rand(n_j, c) * 0.1 + 0.01
    stride = n_j // per_row
    excl = (rs.randint(0, stride, size=(n_i, per_row)) + np.arange(per_row) * stride).astype(np.int32)
    block = 8192
    comp = DeviceCompleter(S, G_col, dtype=dtype)

    def lists(r0, r1):
        return np.arange(r1 - r0 + 1, dtype=np.int64) * per_row, excl[r0:r1].reshape(-1)

    comp.topk(G_row[:block], k, exclude=lists(0, block))                     # warm-up: code objects, scratch
    fused = []
    for _ in range(3):
        t0 = time.perf_counter()
        for r0 in range(0, n_i, block):
            r1 = min(r0 + block, n_i)
            comp.topk(G_row[r0:r1], k, exclude=lists(r0, r1))
        fused.append(time.perf_counter() - t0)

    # the pass alone on resident data
    code, T = comp.code, comp.npd
    m = block
    H = np.dot(G_row[:m], S).astype(T)
    p, i = lists(0, m)
    bh, bp, bi = mem.from_host(H), mem.from_host(p), mem.from_host(i)
    need = C.c_size_t()
    rt.call('skf_complete_topk_workspace_bytes', code, m, n_j, k, 0, C.byref(need))
    ws, oi, ov = mem.empty(need.value), mem.empty(m * k * 4), mem.empty(m * k * comp.es)
    times = []
    for it in range(9):
        mem.synchronize()
        t0 = time.perf_counter()
        rt.call('skf_complete_topk', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, k, bp.ptr, bi.ptr, oi.ptr, k, ov.ptr, k, 0, ws.ptr,
                ws.nbytes, mem.stream)
        mem.synchronize()
        times.append(time.perf_counter() - t0)
    t_block = float(np.median(times[2:]))
    t_kernel = t_block * n_i / m
    t_min = 2.0 * n_i * n_j * c / (PEAK_TFLOPS[dtype] * 1e12)

    # the previous route
    rec = DeviceReconstructor(S, G_col, dtype=dtype)
    hb = 4096
    rec.block(G_row[:hb])
    t0 = time.perf_counter()
    for b in range(host_blocks):
        r0 = b * hb
        X = rec.block(G_row[r0:r0 + hb])
        X[np.repeat(np.arange(hb), per_row), excl[r0:r0 + hb].reshape(-1)] = -np.inf
        part = np.argpartition(-X, k - 1, axis=1)[:, :k]
        order = np.argsort(-np.take_along_axis(X, part, axis=1), axis=1, kind='stable')
        np.take_along_axis(part, order, axis=1)
    t_host = (time.perf_counter() - t0) / (host_blocks * hb) * n_i

    return dict(dtype=dtype, shape=[n_i, n_j], ranks=[c, c], k=k, excluded=n_i * per_row,
                fused_s=round(float(np.median(fused)), 3), fused_s_all=[round(t, 3) for t in fused],
                kernel_block_ms=round(1e3 * t_block, 3), kernel_block_ms_min=round(1e3 * min(times[2:]), 3),
                kernel_block_ms_max=round(1e3 * max(times[2:]), 3), t_kernel_s=round(t_kernel, 4), t_min_s=round(t_min, 4),
                frac=round(t_min / t_kernel, 4), host_route_s=round(t_host, 2),
                host_route_note='measured on %d blocks of %d rows, scaled to %d rows' % (host_blocks, hb, n_i),
                speedup=round(t_host / float(np.median(fused)), 1),
                col_splits_block_8192=chosen_splits(rt, code, block, n_j, k),
                col_splits_m_100000=chosen_splits(rt, code, 100000, n_j, k), col_splits_m_64=chosen_splits(rt, code, 64, n_j, k),
                device_peak_MiB=round(comp.peak_bytes / 2.0 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--dtypes', default='f32,f64')
    ap.add_argument('--shape', default='100000,40000,256,10,800', help='n_i,n_j,rank,k,excluded per row')
    ap.add_argument('--host-blocks', type=int, default=2)
    a = ap.parse_args()
    n_i, n_j, c, k, per_row = [int(v) for v in a.shape.split(',')]
    for dt in a.dtypes.split(','):
        line = json.dumps(run(dt, n_i, n_j, c, k, per_row, a.host_blocks))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
