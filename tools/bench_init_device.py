"""Time of the column-mean initialisers on the device (csrc/skf_init.h) at the config-3 shapes -- 50 000 x 100 000 x 40 000
objects, ranks 128 / 256 / 256, three uniform relations -- and at 1/10 linear scale, per engine, against the host
initialiser (`_init.initialize`) on the same box at 1/10 scale.

    python tools/bench_init_device.py [--scales 10,1] [--dtypes bf16,f32,f64] [--full-dtypes bf16,f32] [--no-host]

One JSON line per measurement:
  where 'device': draw_s (the index shuffles on the host: the random stream, which stays there), pools_s (`random_c` only:
        the norm passes, their read-back, square roots and the stable sort), init_s (selections up, W, the products, the
        epilogue, skf_set_factor, one synchronisation: everything `DeviceInit.apply` does once the pools exist), norms_s (the
        norm pass of the largest relation alone, read-back included);
  where 'host': seconds of `_init.initialize` on host copies of the same relations (1/10 scale only: the full size is
        extrapolated by the caller as gathered elements / measured elements per second, and says so).
`gathered` is the host initialiser's work: sum over the oriented views of n_rows * take * c elements."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

__graft_entry__.build()
import skfusion_amd._native as nat  # noqa: E402
from skfusion_amd._engine import DevicePlan, fill_uniform  # noqa: E402
from skfusion_amd.fusion.decomposition import _init  # noqa: E402

FULL = {'t1': 50000, 't2': 100000, 't3': 40000}
RANKS = {'t1': 128, 't2': 256, 't3': 256}
TYPES = ['t1', 't2', 't3']
PAIRS = [('t1', 't2', 0), ('t1', 't3', 1), ('t2', 't3', 2)]


def gathered(n):
    return sum(n[i] * int(.2 * n[j]) * RANKS[i] + n[j] * int(.2 * n[i]) * RANKS[j] for i, j, _ in PAIRS)


def device(scale, dtype, init_type):
    n = {t: v // scale for t, v in FULL.items()}
    rt = nat.get_runtime()
    rels = [(i, j, fill_uniform((n[i], n[j]), seed, dtype), None) for i, j, seed in PAIRS]
    plan = DevicePlan(TYPES, n, RANKS, rels, [], nat.SKF_DFMF, dtype=dtype)
    plan.synchronize()
    try:
        shapes = {(i, j): (n[i], n[j]) for i, j, _ in PAIRS}
        out = dict(where='device', scale=scale, dtype=dtype, init_type=init_type, gathered=gathered(n))
        for rep in ('warm', 'timed'):                          # (the first pass pays the code-object loads)
            rs = np.random.RandomState(0)
            t0 = time.perf_counter()
            di = _init.DeviceInit(_init.draw_positions(TYPES, RANKS, shapes, init_type, rs), init_type, {})
            t1 = time.perf_counter()
            if init_type == 'random_c':
                for k, (i, j, _) in enumerate(PAIRS):
                    di._pool(plan, k, ((i, j), False))
            t2 = time.perf_counter()
            di.apply(plan, TYPES)
            t3 = time.perf_counter()
            plan.relation_norms(0)
            t4 = time.perf_counter()
        out.update(draw_s=round(t1 - t0, 4), pools_s=round(t2 - t1, 4), init_s=round(t3 - t2, 4), norms_s=round(t4 - t3, 4),
                   device_total_s=round(t3 - t1, 4))
        assert all(np.isfinite(plan.get_factor(t)).all() for t in TYPES[:1])
    finally:
        plan.close()
    print(json.dumps(out), flush=True)


def host(scale, init_type):
    from oracle.dfmf_oracle import hash_uniform_matrix
    n = {t: v // scale for t, v in FULL.items()}
    R = {(i, j): hash_uniform_matrix(seed, n[i], n[j]) for i, j, seed in PAIRS}
    t0 = time.perf_counter()
    _init.initialize(TYPES, n, RANKS, R, init_type, np.random.RandomState(0), {})
    dt = time.perf_counter() - t0
    print(json.dumps(dict(where='host', scale=scale, init_type=init_type, gathered=gathered(n), host_s=round(dt, 3),
                          elements_per_s=round(gathered(n) / dt, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', default='10,1')
    ap.add_argument('--dtypes', default='bf16,f32,f64')
    ap.add_argument('--full-dtypes', default='bf16,f32', help='engines measured at scale 1 (f64 holds 88 GB of relations)')
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    for scale in [int(s) for s in a.scales.split(',')]:
        for dtype in (a.full_dtypes if scale == 1 else a.dtypes).split(','):
            for init_type in ('random_vcol', 'random_c'):
                device(scale, dtype, init_type)
        if scale > 1 and not a.no_host:
            for init_type in ('random_vcol', 'random_c'):
                host(scale, init_type)


if __name__ == '__main__':
    main()
