"""A/B record of the pseudo-inverse (csrc/skf_pinv.h, skf_pinv.inc): one line per case, for ONE library per process.

    SKF_LIB_PATH=<library> python tools/ab_pinv.py             on the GPU
    python tools/ab_pinv.py --emul <emulator library>          on the host emulator (tests/emul)

Stand-alone cases (skf_pinv_sym): sha1 of the bytes of K, the verdict word, the launches of the call -- with no switch set
and with each switch alone at the orders the tests use it at.  Plan cases: workspace bytes, launches per iteration, sha1 of
every G and S after two iterations.  Two builds of the library agree when their outputs are identical (profiles/)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import skfusion_amd._native as nat                                                    # noqa: E402
import pinv_cases                                                                     # noqa: E402

SWITCHES = ('SKF_CHOL_UNBLOCKED=1', 'SKF_CHOL_NO_SMALL=1', 'SKF_PINV_SWEEP=0', 'SKF_SWEEP_BIG=0', 'SKF_SWEEP_STEP_MIN=0',
            'SKF_PINV_JACOBI=1')


def sha(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def switch_applies(switch, n, deficient):
    """The orders the tests of tests/test_emul_kernels.py run each switch at."""
    name = switch.split('=')[0]
    if name == 'SKF_CHOL_UNBLOCKED':
        return n <= 70 and not deficient
    if name == 'SKF_CHOL_NO_SMALL':
        return n <= 70 and not deficient
    if name in ('SKF_PINV_SWEEP', 'SKF_SWEEP_STEP_MIN'):
        return 65 <= n <= 256
    if name == 'SKF_SWEEP_BIG':
        return n > 256
    return n <= 50 or (deficient and n <= 130)             # SKF_PINV_JACOBI


def standalone(rt):
    cases = []
    for n in (1, 2, 5, 33, 50, 64, 65, 96, 130, 256, 257, 300):
        rs = np.random.RandomState(n)
        G = rs.rand(3 * n + 5, n)
        cases.append(('full n=%d f64' % n, nat.SKF_F64, G.T @ G, n, n, False))
    for n in (50, 130):
        rs = np.random.RandomState(n)
        G = rs.rand(3 * n + 5, n)
        cases.append(('full n=%d f32' % n, nat.SKF_F32, G.T @ G, n, n, False))
    for n, rank in ((50, 30), (130, 65), (300, 170)):
        rs = np.random.RandomState(n + rank)
        G = rs.rand(rank, n)
        G[:, n // 2] = G[:, 1]
        cases.append(('rank %d of n=%d f64' % (rank, n), nat.SKF_F64, G.T @ G, n, n, True))
    rs = np.random.RandomState(5)
    Qm, _ = np.linalg.qr(rs.randn(258, 258))
    A = (Qm * np.array([1.0] * 40 + [1e-8] * 2 + [0.0] * 216)) @ Qm.T
    cases.append(('ambiguous n=258 f64', nat.SKF_F64, 0.5 * (A + A.T), 258, 258, True))
    for dtype, tag in ((nat.SKF_F64, 'f64'), (nat.SKF_F32, 'f32')):
        for rank in (None, 20):
            cases.append(('strided n=33 rank %s lda=40 ldk=37 %s' % (rank or 'full', tag), dtype, pinv_cases.strided_matrix(33, rank), 40, 37,
                          rank is not None))
    cases.append(('strided n=70 ldk=72 f64', nat.SKF_F64, pinv_cases.strided_matrix(70), 70, 72, False))
    for name, dtype, A, lda, ldk, deficient in cases:
        n = A.shape[0]
        for switch in ('',) + SWITCHES:
            if switch and not switch_applies(switch, n, deficient):
                continue
            if switch:
                os.environ[switch.split('=')[0]] = switch.split('=')[1]
            try:
                got, pad, verdict, launches = pinv_cases.run_pinv_strided(rt, dtype, A, lda, ldk)
            finally:
                if switch:
                    os.environ.pop(switch.split('=')[0])
            print('%-44s %-22s K=%s pad=%s verdict=%d launches=%d' % (name, switch or '-', sha(got), 'kept' if (pad == pinv_cases.POISON).all()
                                                                       else 'TOUCHED', verdict, launches), flush=True)


def plan_case(rt, name, R, types, rank, G0, dtype, env=None, owned=False):
    from skfusion_amd._engine import DevicePlan, flatten_relations, count_objects, launch_count
    from skfusion_amd.fusion.decomposition._dfmf import owned_plan
    env = env or {}
    os.environ.update(env)
    try:
        rel = flatten_relations(R)
        n = count_objects(types, R)
        if owned:
            plan = owned_plan(nat.SKF_DFMF, rel, [], types, n, rank, dtype, None, 0, 2)
            plan.attach_null_comm(0, 2)
        else:
            plan = DevicePlan(types, n, rank, rel, [], nat.SKF_DFMF, dtype=dtype)
        for t in types:
            plan.set_factor(t, G0[t, t])
        before = launch_count(rt)
        plan.iterate_dist(2) if owned else plan.iterate(2)
        launches = launch_count(rt) - before
        out = [plan.get_factor(t) for t in types] + [plan.get_backbone(k) for k in range(len(rel))]
        ws = plan.workspace_bytes
        plan.close()
    finally:
        for k in env:
            os.environ.pop(k)
    tag = ' '.join('%s=%s' % kv for kv in sorted(env.items())) or '-'
    print('%-44s %-22s ws=%d launches/iteration=%g GS=%s' % ('%s %s' % (name, dtype), tag, ws, launches / 2.0, sha(*out)), flush=True)


def plans(rt):
    from helpers import readme_graph
    R, types, rank = readme_graph()
    rs = np.random.RandomState(3)
    G0 = {(t, t): rs.rand(n, rank[t]) + 0.05 for t, n in zip(types, (50, 100, 40))}
    readme = (R, types, rank, G0)
    rs = np.random.RandomState(5)                     # every rank above 64: the relation pipeline; rank c exceeds its 90 objects
    n = {'a': 100, 'b': 140, 'c': 90}
    rank = {'a': 66, 'b': 128, 'c': 96}
    R = {('a', 'b'): [rs.rand(100, 140)], ('a', 'c'): [rs.rand(100, 90) - 0.3], ('b', 'c'): [rs.rand(140, 90)]}
    pipeline = (R, ['a', 'b', 'c'], rank, {(t, t): rs.rand(n[t], rank[t]) + 0.05 for t in n})
    rs = np.random.RandomState(17)                    # test_emul_engine.py::test_fit_with_a_rank_above_256
    n = {'a': 420, 'b': 150, 'c': 90}
    rank = {'a': 300, 'b': 70, 'c': 40}
    R = {('a', 'b'): [rs.rand(420, 150)], ('a', 'c'): [rs.rand(420, 90) - 0.3], ('b', 'c'): [rs.rand(150, 90)]}
    big = (R, ['a', 'b', 'c'], rank, {(t, t): rs.rand(n[t], rank[t]) + 0.05 for t in n})
    chain = pinv_cases.chain17_graph()
    for dtype in ('f64', 'f32'):
        plan_case(rt, 'readme small-graph', *readme, dtype)
        plan_case(rt, 'readme staged', *readme, dtype, {'SKF_NO_SMALL_FUSED': '1'})
        plan_case(rt, 'pipeline ranks 66/128/96', *pipeline, dtype)
        plan_case(rt, 'ranks 300/70/40', *big, dtype, {'SKF_SWEEP_BIG': '1'})
        plan_case(rt, 'ranks 300/70/40', *big, dtype, {'SKF_SWEEP_BIG': '0'})
        plan_case(rt, 'owned rows 0 of 2, ranks 66/128/96', *pipeline, dtype, owned=True)
        plan_case(rt, 'chain of 17 types', *chain, dtype, {'SKF_NO_SMALL_FUSED': '1'})
    plan_case(rt, 'pipeline ranks 66/128/96', *pipeline, 'bf16')


def main():
    if '--emul' in sys.argv:
        from emul.runtime import HostMemory, use_runtime
        rt = nat.Runtime(nat.load_library(sys.argv[sys.argv.index('--emul') + 1]), HostMemory(), 'emul')
        with use_runtime(rt):
            standalone(rt)
            plans(rt)
    else:
        rt = nat.get_runtime()
        standalone(rt)
        plans(rt)


if __name__ == '__main__':
    main()
