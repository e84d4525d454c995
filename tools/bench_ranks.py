"""Ranks of held-out pairs at BASELINE config 5's shape -- 100 000 users x 40 000 movies, ranks 256 / 256, 10 targets per
row, 80 M excluded (known) pairs -- counted on the device (`_complete.DeviceCompleter.ranks`, csrc/skf_complete.h) against

  (a) `DeviceCompleter.topk` with k = 64 on the same blocks: the same matrix work (2 m n c flop), so it is the yardstick,
  (b) the only route to a rank beyond 64 the project had before: `DeviceReconstructor.block` (what
      `complete_blocks(block_rows=4096)` runs per block) pulled to the host, the known pairs masked, one comparison pass per
      target.

    python tools/bench_ranks.py [--out profiles/r19_ranks.txt] [--dtypes f32,f64] [--host-blocks 2]

Per dtype, JSON lines:
  ranks     whole call path over every row in blocks of 8192 (uploads of the row blocks and their lists, H = G S, the list
            checks, both passes, results back), seconds, median of 3 after a warm-up pass over one block; recall@10,
            recall@100 and MRR of the (random) targets from the ranks;
  topk64    the same for (a); ratio = ranks / topk64;
  kernel    skf_complete_ranks alone on one resident block of 8192 rows, device-synchronised, median of 7 after 2 warm-ups,
            scaled to all rows; frac = t_min / t_kernel with t_min = 2 m n c flop at the dtype's matrix peak; the same for
            skf_complete_topk (k = 64) on that block, and the block again with 1 target per row (what the compare loop
            adds per target shows in the difference);
  host      (b) on the first --host-blocks blocks of 4096 rows, scaled to all rows;
  hub       a block of 8192 rows in which row 0 holds 5 000 targets (157 chunks of 32) next to the block without them:
            what spreading one long row over the chunk grid costs."""
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


def chosen_splits(rt, code, m, n_cols):
    """The column splits of a col_splits = 0 call: the two operators share the decision, and top-k's workspace shows it."""
    need, probe = C.c_size_t(), C.c_size_t()
    rt.call('skf_complete_topk_workspace_bytes', code, m, n_cols, 64, 0, C.byref(need))
    for s in range(1, 33):
        rt.call('skf_complete_topk_workspace_bytes', code, m, n_cols, 64, s, C.byref(probe))
        if probe.value == need.value:
            return s
    return None


def strided(rs, n_i, n_j, per_row):
    """`per_row` ascending columns per row: one in every stride of n_j / per_row."""
    stride = n_j // per_row
    return (rs.randint(0, stride, size=(n_i, per_row)) + np.arange(per_row) * stride).astype(np.int32)


def median_of(fn, runs, warm):
    times = []
    for _ in range(warm + runs):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times[warm:])), times[warm:]


def run(dtype, n_i, n_j, c, per_tgt, per_row, host_blocks, hub):
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
    excl = strided(rs, n_i, n_j, per_row)
    tgt = strided(rs, n_i, n_j, per_tgt)
    block = 8192
    comp = DeviceCompleter(S, G_col, dtype=dtype)

    def lists(a, r0, r1):
        return np.arange(r1 - r0 + 1, dtype=np.int64) * a.shape[1], a[r0:r1].reshape(-1)

    rank = np.empty((n_i, per_tgt), dtype=np.int64)

    def all_ranks():
        for r0 in range(0, n_i, block):
            r1 = min(r0 + block, n_i)
            rank[r0:r1] = comp.ranks(G_row[r0:r1], lists(tgt, r0, r1), exclude=lists(excl, r0, r1))[0].reshape(-1, per_tgt)

    def all_topk():
        for r0 in range(0, n_i, block):
            r1 = min(r0 + block, n_i)
            comp.topk(G_row[r0:r1], 64, exclude=lists(excl, r0, r1))

    comp.ranks(G_row[:block], lists(tgt, 0, block), exclude=lists(excl, 0, block))      # warm-up: code objects, scratch
    comp.topk(G_row[:block], 64, exclude=lists(excl, 0, block))
    t_ranks, ranks_all = median_of(all_ranks, 3, 0)
    t_topk, topk_all = median_of(all_topk, 3, 0)
    pos = rank.reshape(-1)
    metrics = {'recall@10': float((pos < 10).mean()), 'recall@100': float((pos < 100).mean()), 'mrr': float((1.0 / (pos + 1.0)).mean())}

    # the operators alone on resident data
    code, T = comp.code, comp.npd
    m = block
    bh = mem.from_host(np.dot(G_row[:m], S).astype(T))
    xp, xi = [mem.from_host(a) for a in lists(excl, 0, m)]

    def ranks_alone(tl):
        tp, ti = mem.from_host(tl[0]), mem.from_host(tl[1])
        n = len(tl[1])
        need = C.c_size_t()
        rt.call('skf_complete_ranks_workspace_bytes', code, m, n_j, n, 0, C.byref(need))
        ws, orank, oval = mem.empty(need.value), mem.empty(n * 4), mem.empty(n * comp.es)

        def call():
            rt.call('skf_complete_ranks', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, tp.ptr, ti.ptr, n, xp.ptr, xi.ptr, orank.ptr,
                    oval.ptr, 0, ws.ptr, ws.nbytes, mem.stream)
            mem.synchronize()
        mem.synchronize()
        return median_of(call, 7, 2)

    def topk_alone():
        need = C.c_size_t()
        rt.call('skf_complete_topk_workspace_bytes', code, m, n_j, 64, 0, C.byref(need))
        ws, oi, ov = mem.empty(need.value), mem.empty(m * 64 * 4), mem.empty(m * 64 * comp.es)

        def call():
            rt.call('skf_complete_topk', code, bh.ptr, c, m, comp.b.ptr, c, n_j, c, 64, xp.ptr, xi.ptr, oi.ptr, 64, ov.ptr, 64, 0,
                    ws.ptr, ws.nbytes, mem.stream)
            mem.synchronize()
        mem.synchronize()
        return median_of(call, 7, 2)

    tb_ranks, tb_all = ranks_alone(lists(tgt, 0, m))
    tb_one, _ = ranks_alone(lists(tgt[:, :1], 0, m))
    tb_topk, _ = topk_alone()
    t_min = 2.0 * n_i * n_j * c / (PEAK_TFLOPS[dtype] * 1e12)

    # one row with `hub` targets in the block
    ptr = np.arange(m + 1, dtype=np.int64) * per_tgt
    hub_cols = np.sort(rs.choice(n_j, size=hub, replace=False)).astype(np.int32)
    hub_ptr = ptr.copy()
    hub_ptr[1:] += hub - per_tgt
    tb_hub, _ = ranks_alone((hub_ptr, np.concatenate([hub_cols, tgt[1:m].reshape(-1)])))

    # the previous route
    rec = DeviceReconstructor(S, G_col, dtype=dtype)
    hb = 4096
    rec.block(G_row[:hb])
    t0 = time.perf_counter()
    for b in range(host_blocks):
        r0 = b * hb
        X = rec.block(G_row[r0:r0 + hb])
        own = np.take_along_axis(X, tgt[r0:r0 + hb].astype(np.int64), axis=1)
        X[np.repeat(np.arange(hb), per_row), excl[r0:r0 + hb].reshape(-1)] = -np.inf
        for q in range(per_tgt):
            (X > own[:, q:q + 1]).sum(axis=1)
    t_host = (time.perf_counter() - t0) / (host_blocks * hb) * n_i

    return dict(dtype=dtype, shape=[n_i, n_j], ranks=[c, c], targets=n_i * per_tgt, excluded=n_i * per_row,
                ranks_s=round(t_ranks, 3), ranks_s_all=[round(t, 3) for t in ranks_all],
                topk64_s=round(t_topk, 3), topk64_s_all=[round(t, 3) for t in topk_all], ratio_to_topk64=round(t_ranks / t_topk, 3),
                kernel_block_ms=round(1e3 * tb_ranks, 3), kernel_block_ms_min=round(1e3 * min(tb_all), 3),
                kernel_block_ms_max=round(1e3 * max(tb_all), 3), kernel_block_ms_1_target=round(1e3 * tb_one, 3),
                topk64_block_ms=round(1e3 * tb_topk, 3), kernel_ratio_to_topk64=round(tb_ranks / tb_topk, 3),
                t_kernel_s=round(tb_ranks * n_i / m, 4), t_min_s=round(t_min, 4), frac=round(t_min / (tb_ranks * n_i / m), 4),
                hub_targets=hub, hub_block_ms=round(1e3 * tb_hub, 3),
                host_route_s=round(t_host, 2),
                host_route_note='measured on %d blocks of %d rows, scaled to %d rows' % (host_blocks, hb, n_i),
                speedup_over_host=round(t_host / t_ranks, 1), col_splits_block_8192=chosen_splits(rt, code, block, n_j),
                device_peak_MiB=round(comp.peak_bytes / 2.0 ** 20, 1), **metrics)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--dtypes', default='f32,f64')
    ap.add_argument('--shape', default='100000,40000,256,10,800', help='n_i,n_j,rank,targets per row,excluded per row')
    ap.add_argument('--host-blocks', type=int, default=2)
    ap.add_argument('--hub', type=int, default=5000, help='targets of the one long row of the second shape')
    a = ap.parse_args()
    n_i, n_j, c, per_tgt, per_row = [int(v) for v in a.shape.split(',')]
    for dt in a.dtypes.split(','):
        line = json.dumps(run(dt, n_i, n_j, c, per_tgt, per_row, a.host_blocks, a.hub))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
