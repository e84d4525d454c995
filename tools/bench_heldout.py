"""Held-out pairs scored inside the fit, measured on the config-5 shape (bench.py --workload c5: Dfmc, MovieLens-style graph,
ratings 98 % masked) with `--pairs` held-out pairs of the ratings relation among its unknown cells:

  iterations/s of the unmonitored fit;
  iterations/s of the monitored fit at check_every 1 / 8 / 32 (DevicePlan.set_heldout, the monitor's state words read
    between chunks);
  iterations/s of the workaround the monitor replaces: a callback that collects every factor to the host and runs
    DeviceCompleter.entries on the pairs after every iteration;
  the time of one evaluation outside the loop (skf_plan_heldout_sqerr: the H product, the pass and the totals) from events
    on the plan's stream, and the monitor's share of a monitored iteration (monitored - unmonitored).

    python tools/bench_heldout.py [--dtype bf16] [--steps 30] [--warmup 3] [--pairs 1000000] [--scale 1.0]

Prints one JSON line.  The numbers of one run are kept in profiles/heldout.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='bf16', choices=['f32', 'f64', 'bf16'])
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--pairs', type=int, default=1000000)
    ap.add_argument('--scale', type=float, default=1.0)
    ap.add_argument('--workaround-steps', type=int, default=3)
    args = ap.parse_args()

    import torch
    import __graft_entry__
    __graft_entry__.build()
    import bench
    import skfusion_amd._native as nat
    from skfusion_amd._engine import DevicePlan, DeviceCompleter, fill_uniform, launch_count
    from skfusion_amd.fusion.decomposition._dfmf import _collect

    dtype = args.dtype
    types, ranks = bench.C5_TYPES, bench.C5_RANKS
    n = bench.sizes(args.scale, bench.C5_FULL)
    rels, thetas = bench.c5_graph(n, dtype)
    # the held-out pairs: unknown cells of the ratings relation (mask byte 1), their "true" values from the data beneath
    mask = rels[0][3].buf.owner.view(n['user'], n['movie'])
    gen = torch.Generator(device='cuda')
    gen.manual_seed(7)
    flat = torch.randint(0, n['user'] * n['movie'], (int(args.pairs * 1.1),), generator=gen, device='cuda')
    flat = torch.unique(flat[mask.reshape(-1)[flat] != 0])[:args.pairs]
    rows, cols = (flat // n['movie']).cpu().numpy(), (flat % n['movie']).cpu().numpy()
    data = rels[0][2].buf.owner
    tdt = {'bf16': torch.bfloat16, 'f32': torch.float32, 'f64': torch.float64}[dtype]
    vals = data.view(tdt).reshape(-1)[flat].to(torch.float64).cpu().numpy()
    del flat, mask, data

    plan = DevicePlan(types, n, ranks, rels, thetas, nat.SKF_DFMC, dtype=dtype)
    if dtype == 'bf16':
        plan.release_relation_data()
        rels = None
        torch.cuda.empty_cache()

    def reset():
        for k, t in enumerate(types):
            plan.set_factor(t, fill_uniform((n[t], ranks[t]), 100 + k, bench.MASTER[dtype]))

    def timed(run, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0)

    out = {'dtype': dtype, 'n': n, 'pairs': int(rows.size), 'steps': args.steps}
    reset()
    plan.iterate(args.warmup)
    l0 = launch_count()
    out['unmonitored_it_s'] = timed(plan.iterate, args.steps)
    out['unmonitored_launches_per_iter'] = (launch_count() - l0) / float(args.steps)

    def chunks(every):
        def run(steps):
            done = 0
            while done < steps:
                k = min(every, steps - done)
                plan.iterate(k)
                done += k
                plan.monitor(history=False)
        return run
    for every in (1, 8, 32):
        reset()
        plan.set_heldout([(0, rows, cols, vals)], patience=0, capacity=args.steps + args.warmup)
        plan.iterate(args.warmup)
        l0 = launch_count()
        out['monitored_it_s_check_every_%d' % every] = timed(chunks(every), args.steps)
        out['monitored_launches_per_iter'] = (launch_count() - l0) / float(args.steps)
    # one evaluation outside the loop, from events on the plan's stream
    stream = plan.rt.mem._stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    plan.heldout_sqerr()
    reps = 10
    ev[0].record(stream)
    for _ in range(reps):
        plan.rt.call('skf_plan_heldout_sqerr', plan.handle, plan._heldout['out'].ptr, plan.stream)
    ev[1].record(stream)
    torch.cuda.synchronize()
    out['heldout_sqerr_ms'] = ev[0].elapsed_time(ev[1]) / reps
    out['monitor_ms_per_iter_check_every_32'] = 1e3 / out['monitored_it_s_check_every_32'] - 1e3 / out['unmonitored_it_s']
    m = plan.monitor()
    out['best_iter'], out['seen'] = m['best_iter'], m['seen']
    plan.set_heldout([])

    # the workaround: every factor to the host, the pairs scored by a completer that uploads what it needs again
    reset()
    plan.iterate(args.warmup)
    i_rel = [(r[0], r[1], None, None) for r in plan.relations]

    def workaround(steps):
        for _ in range(steps):
            plan.iterate(1)
            G, S = _collect(plan, types, i_rel)
            comp = DeviceCompleter(S['user', 'movie'][0], G['movie', 'movie'], dtype=dtype)
            x = comp.entries(G['user', 'user'], rows, cols)
            float(((vals - x) ** 2).sum())
    out['callback_workaround_it_s'] = timed(workaround, args.workaround_steps)
    plan.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
