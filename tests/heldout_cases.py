"""Held-out pairs scored inside the fit (csrc/skf_heldout.h, skf_plan_set_heldout / skf_plan_heldout_sqerr / the monitor's
getters, DevicePlan.set_heldout, _dfmf.Validation, Dfmf / Dfmc ``validation=``) -- the SAME cases on the host emulator
(tests/test_heldout_emul.py) and on the GPU (tests/test_gpu_heldout.py); every case runs on the current runtime.

1. the operator against host arithmetic: the prediction of every pair has the bits of skf_complete_entries on the same H
   (H1), the total is the f64 sum of ((double)v - (double)x)^2 in the kernel's documented order, bit for bit, and agrees with
   a pure-f64 model of G_i S G_j^T within a bound derived from the data;
2. the refusals of the C ABI; 3. monitoring does not perturb the fit; 4. the history is the truth; 5. the best iterate;
6. the patience mechanics and NaN totals; 7. the API surface."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, launch_count
from skfusion_amd.fusion.decomposition import _dfmf, _dfmc

from guarded import guarded

U = {'f64': 2.0 ** -53, 'f32': 2.0 ** -24, 'bf16': 2.0 ** -24}      # unit round-off of the master type (bf16 plans score on f32 masters)
PATTERNS = ('gaps', 'one_row', 'dups', 'corner')
DEVIATIONS = []                 # (label, |device - f64 model| / bound) of every operator case of this session


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def kernel_order_total(res):
    """The sum of the residuals in the order csrc/skf_heldout.h documents: slabs of 1024 (past the end: +0.0), thread t
    takes ((res[t] + res[t + 256]) + res[t + 512]) + res[t + 768], the 256 sums fold by halves 128, 64, ..., 1, and the
    slabs' partials add up first to last."""
    res = np.asarray(res, dtype=np.float64)
    total = np.float64(0.0)
    for b in range(0, res.size, 1024):
        slab = np.zeros(1024)
        slab[:min(1024, res.size - b)] = res[b:b + 1024]
        a = ((slab[0:256] + slab[256:512]) + slab[512:768]) + slab[768:1024]
        w = 128
        while w > 0:
            a = a[:w] + a[w:2 * w]
            w //= 2
        total = total + a[0]
    return total


def heldout_pairs(rs, n, ni, nj, pattern):
    """(rows, cols) of n held-out pairs, rows non-decreasing: `gaps` -- only every other row has entries; `one_row` -- every
    entry in one row; `dups` -- every pair twice (n odd: one of them three times); `corner` -- the last row and the last
    column present, as the last entry."""
    if pattern == 'one_row':
        return np.full(n, ni // 2, dtype=np.int64), rs.randint(0, nj, n)
    if pattern == 'gaps':
        rows = 2 * rs.randint(0, (ni + 1) // 2, n)
    else:
        rows = rs.randint(0, ni, n)
    cols = rs.randint(0, nj, n)
    if pattern == 'dups' and n > 1:
        h = n // 2
        rows[h:2 * h], cols[h:2 * h] = rows[:h], cols[:h]
        rows[-1], cols[-1] = rows[0], cols[0]
    order = np.argsort(rows, kind='stable')
    rows, cols = rows[order], cols[order]
    if pattern == 'corner':
        rows[-1], cols[-1] = ni - 1, nj - 1
    return rows, cols


def _set_padded(plan, rt, what, k, arr, pad):
    """skf_set_factor / skf_set_backbone from a buffer whose leading dimension is `pad` elements wider than the matrix; the
    padding holds NaN."""
    wide = np.full((arr.shape[0], arr.shape[1] + pad), np.nan, dtype=plan.np_dtype)
    wide[:, :arr.shape[1]] = arr
    buf = rt.mem.from_host(wide)
    rt.call(what, plan.handle, k, buf.ptr, wide.shape[1], plan.stream)
    rt.mem.synchronize()
    return buf


def _entries(rt, code, H, G, rows, cols):
    """skf_complete_entries on host copies of H and G_j (tight leading dimensions)."""
    npd = nat.NP_DTYPE[code]
    hb, gb = rt.mem.from_host(np.ascontiguousarray(H, dtype=npd)), rt.mem.from_host(np.ascontiguousarray(G, dtype=npd))
    rb, cb = rt.mem.from_host(rows.astype(np.int32)), rt.mem.from_host(cols.astype(np.int32))
    out = rt.mem.empty(rows.size * np.dtype(npd).itemsize)
    rt.call('skf_complete_entries', code, hb.ptr, H.shape[1], H.shape[0], gb.ptr, G.shape[1], G.shape[0], G.shape[1], rb.ptr, cb.ptr,
            rows.size, out.ptr, rt.mem.stream)
    rt.mem.synchronize()
    return rt.mem.to_host(out, (rows.size,), npd)


def operator_case(dtype, ni, nj, ci, cj, sizes, label, seed=0):
    """One plan, the lists of `sizes` = [(n, pattern)] attached one after the other; see the module docstring, item 1."""
    rs = np.random.RandomState(seed + 1000 * cj + ci)
    with guarded() as g:
        rt = g.rt
        plan = DevicePlan(['a', 'b'], {'a': ni, 'b': nj}, {'a': ci, 'b': cj}, [('a', 'b', rs.rand(ni, nj), None)], [],
                          nat.SKF_DFMF, dtype=dtype)
        try:
            npd = plan.np_dtype
            Gi, Gj, S = (rs.rand(ni, ci) - 0.3).astype(npd), (rs.rand(nj, cj) - 0.3).astype(npd), (rs.rand(ci, cj) - 0.5).astype(npd)
            keep = [_set_padded(plan, rt, 'skf_set_factor', 0, Gi, 3), _set_padded(plan, rt, 'skf_set_factor', 1, Gj, 5),
                    _set_padded(plan, rt, 'skf_set_backbone', 0, S, 7)]
            Gi64, Gj64, S64 = Gi.astype(np.float64), Gj.astype(np.float64), S.astype(np.float64)
            X = (Gi64 @ S64) @ Gj64.T                                  # the pure-f64 model
            A = (np.abs(Gi64) @ np.abs(S64)) @ np.abs(Gj64).T          # sum of |terms| of every entry
            code = nat.SKF_F64 if dtype == 'f64' else nat.SKF_F32
            for n, pattern in sizes:
                rows, cols = heldout_pairs(rs, n, ni, nj, pattern)
                vals = (X[rows, cols] + 0.25 * rs.randn(n)).astype(npd)
                plan.set_heldout([(0, rows, cols, vals)], capacity=2)
                got = plan.heldout_sqerr()
                assert got.shape == (1,)
                H = plan.heldout_product(0)
                x = _entries(rt, code, H, Gj, rows, cols)             # H1: the bits of skf_complete_entries on the same H
                d = vals.astype(np.float64) - x.astype(np.float64)
                want = kernel_order_total(d * d)
                assert bits(got[0]) == bits(want), '%s n=%d %s: device %r, host order %r' % (label, n, pattern, got[0], want)
                xt = X[rows, cols]
                b = (ci + cj + 4) * U[dtype] * A[rows, cols]
                dm = vals.astype(np.float64) - xt
                model = float((dm * dm).sum())
                bound = float((b * (2 * np.abs(dm) + b)).sum()) + n * 2.0 ** -52 * model
                dev = abs(float(got[0]) - model)
                DEVIATIONS.append(('%s %s c_j=%d n=%d %s' % (label, dtype, cj, n, pattern), dev / bound if bound else 0.0))
                print('heldout operator %s %s c_j=%d n=%d %s: |device - f64 model| = %.3e, bound %.3e' % (label, dtype, cj, n, pattern, dev, bound))
                assert dev <= bound, (label, n, pattern, dev, bound)
            del keep
        finally:
            plan.close()


ALL_N = (1, 3, 4, 1023, 1024, 1025, 2500)


def sizes_for(cj):
    """Every n of the issue with the patterns in rotation (the rotation starts at a different pattern for every c_j), and
    all four patterns at n = 1025 (more than one slab, a ragged last one)."""
    k = cj % 4
    return [(n, PATTERNS[(q + k) % 4]) for q, n in enumerate(ALL_N)] + [(1025, p) for p in PATTERNS]


# ---- 2. refusals at the C ABI ------------------------------------------------------------------------------------------------
def refusals_case():
    rs = np.random.RandomState(5)
    ni, nj, ci, cj = 37, 41, 5, 7
    with guarded() as g:
        rt = g.rt
        plan = DevicePlan(['a', 'b'], {'a': ni, 'b': nj}, {'a': ci, 'b': cj}, [('a', 'b', rs.rand(ni, nj), None)], [], nat.SKF_DFMF, dtype='f64')
        fold = DevicePlan(['a', 'b'], {'a': ni, 'b': nj}, {'a': ci, 'b': cj}, [('a', 'b', rs.rand(ni, nj), None)], [], nat.SKF_TRANSFORM,
                          dtype='f64', target='a')
        try:
            plan.set_factors({'a': rs.rand(ni, ci), 'b': rs.rand(nj, cj)})
            plan.set_backbone(0, rs.rand(ci, cj))
            n = 10
            rows, cols, vals = np.sort(rs.randint(0, ni, n)).astype(np.int32), rs.randint(0, nj, n).astype(np.int32), rs.rand(n)
            good = [rt.mem.from_host(a) for a in (rows, cols, vals)]

            def desc(lists):
                d = (nat.HeldoutDesc * len(lists))()
                for l, (rel, cnt, bufs) in enumerate(lists):
                    d[l].rel, d[l].n = rel, cnt
                    d[l].rows, d[l].cols, d[l].values = bufs[0].ptr, bufs[1].ptr, bufs[2].ptr
                return d
            need = C.c_size_t()
            rt.call('skf_plan_heldout_workspace_bytes', plan.handle, 1, desc([(0, n, good)]), 4, C.byref(need))
            ws = rt.mem.empty(need.value)
            out = rt.mem.from_host(np.full(4, 7.5))

            def variant(which, values):
                a = [rows.copy(), cols.copy(), vals.copy()]
                a[which][:] = values
                return [rt.mem.from_host(x) for x in a]
            dec = rows.copy()
            dec[0], dec[1] = ni - 1, 0
            col_hi = cols.copy()
            col_hi[n // 2] = nj
            nan = vals.copy()
            nan[n - 1] = np.nan
            cases = [('decreasing rows', plan, 1, [(0, n, variant(0, dec))], need.value),
                     ('a column equal to n_j', plan, 1, [(0, n, variant(1, col_hi))], need.value),
                     ('a NaN value', plan, 1, [(0, n, variant(2, nan))], need.value),
                     ('n = 0', plan, 1, [(0, 0, good)], need.value),
                     ('two lists on one relation', plan, 2, [(0, n, good), (0, n, good)], need.value),
                     ('a transform plan', fold, 1, [(0, n, good)], need.value),
                     ('a workspace one byte short', plan, 1, [(0, n, good)], need.value - 1)]
            for what, pl, n_lists, lists, nbytes in cases:
                rc = rt.lib.skf_plan_set_heldout(pl.handle, n_lists, desc(lists), 0, 0.0, 4, ws.ptr, nbytes, pl.stream)
                assert rc in (nat.SKF_E_INVALID, nat.SKF_E_STATE), (what, rc)
                assert rt.lib.skf_last_error()
                # the plan stays unmonitored: nothing to score, nothing to read, nothing written to the outputs
                assert rt.lib.skf_plan_heldout_sqerr(pl.handle, out.ptr, pl.stream) == nat.SKF_E_STATE, what
                assert rt.lib.skf_plan_get_monitor(pl.handle, None, None, None, None, None, None, 0, pl.stream) == nat.SKF_E_STATE, what
                assert rt.lib.skf_get_best_factor(pl.handle, 0, out.ptr, ci, pl.stream) == nat.SKF_E_STATE, what
                rt.mem.synchronize()
                assert (rt.mem.to_host(out, (4,), np.float64) == 7.5).all(), what
            # ... and a refusal detaches a monitor that was attached before it
            rt.call('skf_plan_set_heldout', plan.handle, 1, desc([(0, n, good)]), 0, 0.0, 4, ws.ptr, need.value, plan.stream)
            assert rt.lib.skf_plan_heldout_sqerr(plan.handle, out.ptr, plan.stream) == nat.SKF_OK
            assert rt.lib.skf_get_best_factor(plan.handle, 0, out.ptr, ci, plan.stream) == nat.SKF_E_STATE      # nothing judged yet
            assert rt.lib.skf_plan_set_heldout(plan.handle, 1, desc([(0, 0, good)]), 0, 0.0, 4, ws.ptr, need.value, plan.stream) == nat.SKF_E_INVALID
            assert rt.lib.skf_plan_heldout_sqerr(plan.handle, out.ptr, plan.stream) == nat.SKF_E_STATE
            rt.mem.synchronize()
        finally:
            plan.close()
            fold.close()


# ---- the tiny completion graph of items 3, 4 and 6 ---------------------------------------------------------------------------
TYPES = ['a', 'b', 'c']
N_OBJ = {'a': 70, 'b': 50, 'c': 33}
RANKS_SMALL = {'a': 5, 'b': 4, 'c': 3}
RANKS_WIDE = {'a': 20, 'b': 64, 'c': 8}
# kernel launches of the UNMONITORED 12-iteration f64 fit of tiny_graph below (launch_count around _dfmc.dfmc), measured on
# the commit before this feature existed: the feature leaves an unmonitored plan's launches alone.  Keyed by
# (ranks of a / b / c, SKF_NO_SMALL_FUSED set).
PARENT_LAUNCHES = {((5, 4, 3), False): 338, ((20, 64, 8), False): 338, ((5, 4, 3), True): 338, ((20, 64, 8), True): 338}


def tiny_graph(ranks, seed=3):
    """70 x 50 with 40 % of its cells known (the rest masked: unknown) and 50 x 33 without a mask; G0; and 300 held-out pairs
    of the first relation among its UNKNOWN cells with planted values."""
    rs = np.random.RandomState(seed)
    A, B, Cm = rs.rand(70, 3), rs.rand(50, 3), rs.rand(33, 3)
    R1 = A @ B.T + 0.05 * rs.randn(70, 50)
    R2 = B @ Cm.T + 0.05 * rs.randn(50, 33)
    mask = rs.rand(70, 50) > 0.4                                   # True = unknown
    R = {('a', 'b'): [np.where(mask, 0.0, R1)], ('b', 'c'): [R2]}
    M = {('a', 'b'): [mask], ('b', 'c'): [None]}
    G0 = {(t, t): rs.rand(N_OBJ[t], ranks[t]) for t in TYPES}
    unknown = np.flatnonzero(mask.reshape(-1))
    pick = np.sort(rs.choice(unknown, 300, replace=False))
    rows, cols = pick // 50, pick % 50
    return R, M, G0, (rows, cols, R1[rows, cols])


def fit_tiny(ranks, max_iter, validation=None, dtype='f64', variant='dfmc', **kw):
    R, M, G0, _ = tiny_graph(ranks)
    if variant == 'dfmf':
        return _dfmf.dfmf(R, {}, TYPES, ranks, max_iter=max_iter, G0=G0, dtype=dtype, validation=validation, **kw)
    return _dfmc.dfmc(R, M, {}, TYPES, ranks, max_iter=max_iter, G0=G0, dtype=dtype, validation=validation, **kw)


def unmonitored_launches(ranks, max_iter=12):
    """Launches of the unmonitored fit (nothing here names the feature: the same statement runs on the commit before it)."""
    R, M, G0, _ = tiny_graph(ranks)
    before = launch_count()
    _dfmc.dfmc(R, M, {}, TYPES, ranks, max_iter=max_iter, G0=G0, dtype='f64')
    return launch_count() - before


def tiny_validation(ranks, **kw):
    held = tiny_graph(ranks)[3]
    return _dfmf.Validation([(('a', 'b'), ) + held], **kw)


def same_model(one, two):
    (G1, S1), (G2, S2) = one, two
    assert sorted(G1, key=str) == sorted(G2, key=str) and sorted(S1, key=str) == sorted(S2, key=str)
    for k in G1:
        assert G1[k].tobytes() == G2[k].tobytes(), k
    for k in S1:
        assert len(S1[k]) == len(S2[k])
        for a, b in zip(S1[k], S2[k]):
            assert a.tobytes() == b.tobytes(), k


def no_perturbation_case(ranks, forced, monkeypatch):
    """3.: 12 monitored iterations with restore_best=False leave the factors and backbones of the unmonitored fit, byte for
    byte; the unmonitored fit issues the launches it issued before the feature existed."""
    if forced:
        monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    plain_launches = unmonitored_launches(ranks)
    plain = fit_tiny(ranks, 12)
    v = tiny_validation(ranks, restore_best=False, check_every=5)
    watched = fit_tiny(ranks, 12, validation=v)
    same_model(plain, watched)
    assert v.n_iter == 12 and v.sqerr.shape == (12, 1) and not v.stopped and 1 <= v.best_iter <= 12
    key = (tuple(ranks[t] for t in TYPES), bool(forced))
    print('unmonitored launches', key, plain_launches)
    assert plain_launches == PARENT_LAUNCHES[key], (key, plain_launches)


def history_case(ranks, dtype='f64'):
    """4.: row t - 1 of the history of ONE monitored fit is heldout_sqerr of an unmonitored fit of t iterations, bit for bit;
    two monitored runs give the same bits."""
    v = tiny_validation(ranks, restore_best=False)
    fit_tiny(ranks, 6, validation=v, dtype=dtype)
    again = tiny_validation(ranks, restore_best=False, check_every=1)
    fit_tiny(ranks, 6, validation=again, dtype=dtype)
    assert v.sqerr.shape == (6, 1) and v.sqerr.tobytes() == again.sqerr.tobytes()
    R, M, G0, held = tiny_graph(ranks)
    for t in range(1, 7):
        G, S = fit_tiny(ranks, t, dtype=dtype)
        assert bits(final_sqerr(ranks, R, M, G, S, held, dtype)) == bits(v.sqerr[t - 1, 0]), t


def final_sqerr(ranks, R, M, G, S, held, dtype):
    """heldout_sqerr of a fitted model: the model set into a fresh plan (skf_set_factor / skf_set_backbone), no iteration."""
    rel_list = [('a', 'b', R['a', 'b'][0], M['a', 'b'][0]), ('b', 'c', R['b', 'c'][0], None)]
    plan = DevicePlan(TYPES, N_OBJ, ranks, rel_list, [], nat.SKF_DFMC, dtype=dtype)
    try:
        plan.set_factors({t: G[t, t] for t in TYPES})
        plan.set_backbone(0, S['a', 'b'][0])
        plan.set_backbone(1, S['b', 'c'][0])
        plan.set_heldout([(0,) + tuple(held)])
        return plan.heldout_sqerr()[0]
    finally:
        plan.close()


# ---- 5. the best iterate ---------------------------------------------------------------------------------------------------
BEST_SEED = 0           # pinned on the emulator: best_graph(BEST_SEED) has its first minimum strictly inside (1, BEST_ITERS)
BEST_ITERS = 40
BEST_RANKS = {'u': 20, 'v': 20, 'w': 20}
BEST_N = {'u': 60, 'v': 50, 'w': 30}


def best_graph(seed=BEST_SEED):
    """Planted rank-3 data plus noise, fitted at ranks 20 / 20 / 20: 10 % of u x v known, 5 % held out, the rest unknown."""
    rs = np.random.RandomState(seed)
    A, B, Cm = rs.rand(60, 3), rs.rand(50, 3), rs.rand(30, 3)
    R1 = A @ B.T + 0.3 * rs.randn(60, 50)
    R2 = B @ Cm.T + 0.3 * rs.randn(50, 30)
    draw = rs.rand(60, 50)
    mask = draw >= 0.10                                            # True = unknown
    held = np.flatnonzero(((draw >= 0.10) & (draw < 0.15)).reshape(-1))
    rows, cols = held // 50, held % 50
    R = {('u', 'v'): [np.where(mask, 0.0, R1)], ('v', 'w'): [R2]}
    M = {('u', 'v'): [mask], ('v', 'w'): [None]}
    G0 = {(t, t): rs.rand(BEST_N[t], 20) for t in ('u', 'v', 'w')}
    return R, M, G0, (rows, cols, R1[rows, cols])


def fit_best(max_iter, validation=None, seed=BEST_SEED):
    R, M, G0, _ = best_graph(seed)
    return _dfmc.dfmc(R, M, {}, ['u', 'v', 'w'], BEST_RANKS, max_iter=max_iter, G0=G0, dtype='f64', validation=validation)


def best_history(seed=BEST_SEED):
    v = _dfmf.Validation([(('u', 'v'),) + best_graph(seed)[3]], restore_best=True)
    model = fit_best(BEST_ITERS, v, seed)
    return v, model


def interior_minimum(total):
    """The precondition of item 5: the first minimum of the pooled history lies strictly inside (1, max_iter)."""
    k = int(np.argmin(total))
    return 0 < k < total.size - 1


def best_iterate_case():
    v, model = best_history()
    total = v.sqerr.sum(axis=1)
    assert interior_minimum(total), 'precondition: the held-out error of the pinned case has no interior minimum: %r' % (total,)
    assert v.best_iter == int(np.argmin(total)) + 1 and not v.stopped and v.n_iter == BEST_ITERS
    same_model(model, fit_best(v.best_iter))


# ---- 6. patience mechanics ---------------------------------------------------------------------------------------------------
def patience_case(ranks, max_iter=12):
    first = fit_tiny(ranks, 1)
    models = []
    for check_every in (1, 3, 8):
        v = tiny_validation(ranks, patience=3, min_delta=np.inf, check_every=check_every)
        models.append(fit_tiny(ranks, max_iter, validation=v))
        assert v.best_iter == 1 and v.stopped
        assert v.sqerr.shape == (4, 1)                              # the judge stopped at iteration 4
        assert v.n_iter == min(max_iter, -(-4 // check_every) * check_every), (check_every, v.n_iter)
        same_model(models[-1], first)
    assert models[0][0]['a', 'a'].tobytes() == models[2][0]['a', 'a'].tobytes()


def alongside_case(ranks):
    """`callback`, `stopping` and `compute_err` keep working beside the monitor, through the host loop with a chunk of one:
    the same history and model, the callback once per iteration run, and n_iter at the stop iteration itself."""
    alone = tiny_validation(ranks, restore_best=False)
    model = fit_tiny(ranks, 6, validation=alone)
    calls = []
    beside = tiny_validation(ranks, restore_best=False)
    same_model(model, fit_tiny(ranks, 6, validation=beside, callback=lambda G, S, it: calls.append(it), compute_err=True))
    assert calls == list(range(6)) and beside.n_iter == 6 and beside.sqerr.tobytes() == alone.sqerr.tobytes()
    calls = []
    v = tiny_validation(ranks, patience=3, min_delta=np.inf)
    same_model(fit_tiny(ranks, 12, validation=v, callback=lambda G, S, it: calls.append(it)), fit_tiny(ranks, 1))
    assert v.stopped and v.best_iter == 1 and v.n_iter == 4 and calls == [0, 1, 2, 3] and v.sqerr.shape == (4, 1)


def nan_case():
    """A NaN held-out total never improves: NaN in a factor, heldout_sqerr answers NaN, and one monitored iteration leaves the
    monitor without a best iterate."""
    ranks = RANKS_SMALL
    R, M, G0, held = tiny_graph(ranks)
    rel_list = [('a', 'b', R['a', 'b'][0], M['a', 'b'][0]), ('b', 'c', R['b', 'c'][0], None)]
    with guarded():
        plan = DevicePlan(TYPES, N_OBJ, ranks, rel_list, [], nat.SKF_DFMC, dtype='f64')
        try:
            bad = G0['b', 'b'].copy()
            bad[int(held[1][0]), 1] = np.nan
            plan.set_factors({'a': G0['a', 'a'], 'b': bad, 'c': G0['c', 'c']})
            plan.set_backbone(0, np.ones((ranks['a'], ranks['b'])))
            plan.set_backbone(1, np.ones((ranks['b'], ranks['c'])))
            plan.set_heldout([(0,) + tuple(held)], patience=0, capacity=4)
            assert np.isnan(plan.heldout_sqerr()[0])
            plan.iterate(0)
            assert plan.monitor()['seen'] == 0
            plan.iterate(1)
            m = plan.monitor()
            assert m['seen'] == 1 and m['best_iter'] == 0 and not m['stopped'] and m['best'] == np.inf
            assert np.isnan(m['history'][0, 0])
            with pytest.raises(nat.SkfNativeError) as err:
                plan.best_factor('a')
            assert err.value.code == nat.SKF_E_STATE
        finally:
            plan.close()


# ---- 7. API surface --------------------------------------------------------------------------------------------------------
def api_graph(ranks=(5, 4, 3), seed=11, masked='sparse'):
    """users x movies with missing values (`masked`: a scipy.sparse relation with unstored='unknown', or a MaskedArray),
    movies x genres dense; held-out pairs of both relations (those of the first among its unknown cells)."""
    from skfusion_amd.fusion import FusionGraph, Relation, ObjectType
    rs = np.random.RandomState(seed)
    n_u, n_m, n_g = 60, 45, 20
    A, B, Cm = rs.rand(n_u, 3), rs.rand(n_m, 3), rs.rand(n_g, 3)
    full = A @ B.T + 0.05 * rs.randn(n_u, n_m)
    draw = rs.rand(n_u, n_m)
    known = draw < 0.3
    held = np.flatnonzero(((draw >= 0.3) & (draw < 0.4)).reshape(-1))
    h_rows, h_cols = held // n_m, held % n_m
    users, movies, genres = ObjectType('users', ranks[0]), ObjectType('movies', ranks[1]), ObjectType('genres', ranks[2])
    if masked == 'sparse':
        kr, kc = np.nonzero(known)
        data = scipy.sparse.csr_matrix((full[kr, kc], (kr, kc)), shape=full.shape)
        ratings = Relation(data, users, movies, name='ratings', unstored='unknown')
    else:
        ratings = Relation(np.ma.MaskedArray(full, mask=~known), users, movies, name='ratings')
    G2 = B @ Cm.T + 0.05 * rs.randn(n_m, n_g)
    tags = Relation(G2, movies, genres, name='genres')
    t_rows, t_cols = rs.randint(0, n_m, 40), rs.randint(0, n_g, 40)
    held1 = (h_rows, h_cols, full[h_rows, h_cols])
    held2 = (t_rows, t_cols, G2[t_rows, t_cols] + 0.01)
    return FusionGraph([ratings, tags]), ratings, tags, held1, held2, known


def api_formats_case(cls_name='Dfmc'):
    from skfusion_amd import fusion
    cls = getattr(fusion, cls_name)
    hist = []
    for fmt in ('csr', 'csc', 'coo', 'tuple'):
        graph, ratings, tags, held1, held2, _ = api_graph()
        if fmt == 'tuple':
            held = held1
        else:
            m = scipy.sparse.coo_matrix((held1[2], (held1[0], held1[1])), shape=ratings.data.shape)
            held = {'csr': m.tocsr(), 'csc': m.tocsc(), 'coo': m}[fmt]
        fit = cls(max_iter=6, init_type='random_vcol', random_state=0, validation=[(ratings, held)]).fuse(graph)
        assert fit.validation_sqerr_[0].shape == (6, 1) and fit.n_iter_ == [6] and fit.stopped_early_ == [False]
        assert np.allclose(fit.validation_rmse_[0], np.sqrt(fit.validation_sqerr_[0][:, 0] / held1[0].size), rtol=0, atol=0)
        hist.append(fit.validation_sqerr_[0])
    # (the class layer orders the pairs by row, then column: whatever order a format stores them in, the same list)
    for h in hist[1:]:
        assert h.tobytes() == hist[0].tobytes()


def api_two_lists_and_runs_case():
    from skfusion_amd.fusion import Dfmc
    graph, ratings, tags, held1, held2, _ = api_graph()
    both = Dfmc(max_iter=5, init_type='random_vcol', random_state=0, n_run=2, validation=[(ratings, held1), (tags, held2)],
                restore_best=False).fuse(graph)
    assert len(both.validation_sqerr_) == 2 and len(both.best_iter_) == 2 and both.n_iter_ == [5, 5]
    for run in range(2):
        h = both.validation_sqerr_[run]
        assert h.shape == (5, 2)
        pooled = h.sum(axis=1)
        assert both.best_iter_[run] == int(np.argmin(pooled)) + 1                       # the criterion is the pooled sum
        assert np.array_equal(both.validation_rmse_[run], np.sqrt(pooled / (held1[0].size + held2[0].size)))
    assert both.validation_sqerr_[0].tobytes() != both.validation_sqerr_[1].tobytes()    # another restart, another G0
    # each list alone gives its column
    one = Dfmc(max_iter=5, init_type='random_vcol', random_state=0, n_run=2, validation=[(tags, held2)], restore_best=False).fuse(graph)
    for run in range(2):
        assert one.validation_sqerr_[run][:, 0].tobytes() == both.validation_sqerr_[run][:, 1].tobytes()
    # the plain fit: the same models (restore_best=False), every new attribute None
    plain = Dfmc(max_iter=5, init_type='random_vcol', random_state=0, n_run=2).fuse(graph)
    for name in ('validation_sqerr_', 'validation_rmse_', 'best_iter_', 'n_iter_', 'stopped_early_'):
        assert getattr(plain, name) is None
    for run in range(2):
        for ot in graph.object_types:
            assert plain.factor(ot, run).tobytes() == both.factor(ot, run).tobytes()
        for rel in (ratings, tags):
            assert plain.backbone(rel, run).tobytes() == both.backbone(rel, run).tobytes()


def api_dfmf_case():
    """Dfmf as well as Dfmc: dense relations, early stopping through the class layer, the best iterate returned."""
    from skfusion_amd.fusion import Dfmf, FusionGraph, Relation, ObjectType
    rs = np.random.RandomState(2)
    a, b = ObjectType('a', 6), ObjectType('b', 5)
    full = rs.rand(40, 3) @ rs.rand(3, 30) + 0.2 * rs.randn(40, 30)
    rel = Relation(full, a, b, name='ab')
    graph = FusionGraph([rel])
    rows, cols = rs.randint(0, 40, 80), rs.randint(0, 30, 80)
    held = (rows, cols, full[rows, cols] + 0.2 * rs.randn(80))
    fit = Dfmf(max_iter=30, init_type='random_vcol', random_state=1, validation=[(rel, held)], patience=2, min_delta=np.inf,
               check_every=4).fuse(graph)
    assert fit.best_iter_ == [1] and fit.stopped_early_ == [True] and fit.n_iter_ == [4] and fit.validation_sqerr_[0].shape == (3, 1)
    ref = Dfmf(max_iter=1, init_type='random_vcol', random_state=1).fuse(graph)
    assert fit.factor(a).tobytes() == ref.factor(a).tobytes() and fit.backbone(rel).tobytes() == ref.backbone(rel).tobytes()


def api_refusals_case():
    from skfusion_amd.fusion import Dfmc, Dfmf, Relation, ObjectType
    from skfusion_amd.fusion.base import DataFusionError

    def fails(exc, match, **kw):
        graph = kw.pop('graph')
        with pytest.raises(exc, match=match):
            Dfmc(max_iter=3, init_type='random_vcol', random_state=0, **kw).fuse(graph)
    graph, ratings, tags, held1, held2, known = api_graph()
    stranger = Relation(np.ones((60, 45)), ratings.row_type, ratings.col_type, name='other')
    fails(DataFusionError, r'R_\(users,movies\)', graph=graph, validation=[(stranger, held1)])
    graph2, ratings2, tags2, _, h2, _ = api_graph()
    tags2.preprocessor = lambda x: x
    fails(ValueError, r'R_\(movies,genres\).*preprocessor', graph=graph2, validation=[(tags2, h2)])
    fails(ValueError, r"shard='runs'", graph=graph, validation=[(ratings, held1)], shard='rows')
    out = (np.array([0, 60]), np.array([0, 0]), np.array([1.0, 1.0]))
    fails(ValueError, r'R_\(users,movies\).*outside', graph=graph, validation=[(ratings, out)])
    out = (np.array([0, 1]), np.array([0, -1]), np.array([1.0, 1.0]))
    fails(ValueError, r'R_\(users,movies\).*outside', graph=graph, validation=[(ratings, out)])
    inf = (held1[0], held1[1], np.where(np.arange(held1[0].size) == 3, np.inf, held1[2]))
    fails(ValueError, r'R_\(users,movies\).*not finite', graph=graph, validation=[(ratings, inf)])
    fails(ValueError, r'patience without validation', graph=graph, patience=3)
    fails(ValueError, r'two held-out lists', graph=graph, validation=[(ratings, held1), (ratings, held1)])
    # a held-out pair the training relation knows: both masked forms
    kr, kc = np.nonzero(known)
    leak = (np.append(held1[0], kr[0]), np.append(held1[1], kc[0]), np.append(held1[2], 1.0))
    fails(ValueError, r'R_\(users,movies\).*known to the training relation', graph=graph, validation=[(ratings, leak)])
    graph_m, ratings_m, _, held_m, _, known_m = api_graph(masked='array')
    fails(ValueError, r'R_\(users,movies\).*known to the training relation', graph=graph_m, validation=[(ratings_m, leak)])
    # ... and the masked array is accepted on its unknown cells; plain arrays and unstored='zero' cannot be checked
    ok = Dfmc(max_iter=3, init_type='random_vcol', random_state=0, validation=[(ratings_m, held_m)]).fuse(graph_m)
    assert ok.validation_sqerr_[0].shape == (3, 1)
    ok = Dfmf(max_iter=3, init_type='random_vcol', random_state=0, validation=[(tags, held2)]).fuse(graph)
    assert ok.validation_sqerr_[0].shape == (3, 1)
