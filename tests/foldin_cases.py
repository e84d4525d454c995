"""The fold-in (SKF_TRANSFORM: DfmfTransform, _dfmf.transform / transform_runs) held to a host model of one iteration,
stage by stage -- the sibling of dense_cases.py (fits) and known_cases.py (known-entry lists).  The same cases run on the
host emulator (tests/test_emul_engine.py, `fold_in`) and on the GPU (tests/test_gpu_foldin_model.py).  Only the target
type moves; the partner factors and the backbones are frozen, so everything that does not depend on the target's factor
is formed once (prepare_transform, csrc/skf_schedule.inc) and an iteration is one update.  Every stage is checked on the
DEVICE's own inputs to it:

  1. contractions  P = R G_j (target on the row side), Q = R^T G_i (target on the column side) against the frozen partner
                   factor (relation_gemm / bitmap / row gathers)
  2. one step      G1 = G0 o sqrt(E / max(D, eps)),  E = Ec + G0 Bn (+ Theta- G0),  D = Dc + G0 Bp (+ Theta+ G0), where
                   Ec, Dc = sum (P S^T)+-, (Q S)+-  and  Bn, Bp = sum B-+ with B = S Gram_j S^T (row side) or
                   S^T Gram_i S (column side), each relation split before the sum (reference _dfmf.py:385-428) -- on the
                   host from the device's P / Q, the host S and the f64 Gram matrices of the device's partner factors.
                   Fused path (foldin_step_kernel: no constraint on the target, MFMA engine): one launch per iteration;
                   generic path (iterate_transform otherwise): G Bn / G Bp with EPI_ACC, the constraint terms,
                   mult_update and, bf16, the G^T refresh that the next iteration's constraint product reads
  3. later steps   each on the device's previous output; iterate(k) gives the bits of k calls of iterate(1)
  4. re-preparation  after skf_set_backbone of one relation and after skf_set_factor of a partner type, the next
                   iteration is the model's with the new S / the new partner factor (stale Ec / Dc / B sums fail it)
  5. relation_sqerr  sum (R - G_i S G_j^T)^2 of every new relation against the f64 host sum

Error model.  The host repeats the engine's operand roundings and nothing else -- f64: none; f32: relation, factors, P,
Q, Ec, Dc in f32; bf16: the one bf16 copy of R (0 / 1 relations exact), bf16 partner G^T (or bf16 factor rows) in the
contractions, bf16 constraint halves against the stored bf16 G^T of the target in a dense constraint product, f32
everywhere else.  S is handed to the f32 / bf16 engines already rounded to f32, so host and device hold the same S.  The
Gram matrices and the B products are f64 in every engine.  What remains is bounded element by element, as in
dense_cases.py (a)-(e):
  (a) an accumulation of k products in unit u (2^-53 for f64, 2^-24 for f32 accumulation) moves an element by at most
      (k + 2) u (|X| |Y|) -- k = n_partner (+ split-K partials, 8 at most) for P and Q, c_partner for P S^T and Q S, c_t
      for G B, n_t (or the non-zeros of the row) for Theta G; every stored or accumulated result adds u_m |value|;
  (b) the +- split is 1-Lipschitz: an element of A near zero that flips sign moves at most its own error between E and D;
  (c) the device's B is f64 from the same S and the f64 Gram of the same factor: the host's is off by at most
      (c + n + 4) u64 |S| |Gram| |S|^T;
  (d) E and D are sums of non-negative terms, so  |dG1| / G1 <= 1/2 (|dE| / E + |dD| / D) + 3 u_m;
  (e) the one rounding specific to the fused kernel: Bn / Bp are rounded to the master type while staged (u_m |B|) --
      the rounding the generic path's mixed-precision product makes too, so one bound serves both paths.
relation_sqerr: the reconstruction as dense_cases.Model.completion forms it (bf16: H = G_i S and G_j rounded to bf16, with
the band of dense_cases (e)), and the sum of squares adds (n_i + n_j + 10) max(u, u64) of itself (a sum of non-negative
terms whose reduction depth is below n_i + n_j).  Each bound is known_cases.K_SAFE times the first-order sum; every check
goes through helpers.within."""
import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan, upload_graph, small_graph_limits
from helpers import within
from known_cases import K_SAFE, U_ACC, store_round
from dense_cases import U64, U_M, EPS, Model as DenseModel, constraint, neg, pos, ratio, relation

MFMA, VALU = nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU
GATHER_RANKS = (64, 128, 256)           # skf_api.hip: 0 / 1 relations as lists over bf16 factor rows at these ranks ...
GATHER_PER = 80                         # ... with at most one entry in 80 set
# engine name: (dtype, skf engine)
ENGINES = {'f64': ('f64', MFMA), 'f32': ('f32', MFMA), 'bf16': ('bf16', MFMA), 'f64_valu': ('f64', VALU),
           'f32_valu': ('f32', VALU)}


def kernel_of(engine, n_t, c_t, theta):
    """The iteration the schedule runs (fold_fused / fold_steps, csrc/skf_schedule.inc).  A RESTATEMENT of the
    schedule's dispatch rule, not an observation: it keeps each case's label honest about the shape it needs; of the
    device's choice only fused vs generic is observed (plan.batchable()), not which foldin_step_kernel instantiation ran."""
    dt, eng = ENGINES[engine]
    if eng != MFMA or theta is not None:
        return 'generic'
    if dt == 'f64':
        return 'f64<2,2,16>' if n_t > 64 and c_t > 64 else 'f64<1,1,16>'
    return 'f32<1,1,16>'


# ---- the graph --------------------------------------------------------------------------------------------------------
def fold_graph(n, rels, theta, rs):
    """rels: [(side, partner, kind)] with side 'row' (the target is the row type) or 'col'; a pair may come twice.
    Returns [(row type, col type, R)] and the target's constraint (or None)."""
    out = []
    for side, o, kind in rels:
        if side == 'row':
            out.append(('t', o, relation(kind, n['t'], n[o], rs)))
        else:
            out.append((o, 't', relation(kind, n[o], n['t'], rs)))
    return out, (constraint(theta, n['t'], rs) if theta else None)


def frozen_model(dt, n, ranks, rel_list, rs):
    """One fitted model to fold into: partner factors, backbones of both signs (both sides of every split populated;
    f32 / bf16 engines: rounded to f32, as the device holds them), and a start G0 of the target."""
    Gp = {o: rs.rand(n[o], ranks[o]) + 0.1 for o in sorted(n) if o != 't'}
    S = [rs.rand(ranks[i], ranks[j]) * 2.0 - 0.6 for i, j, _ in rel_list]
    if dt != 'f64':
        S = [store_round(s, 'f32') for s in S]
    return Gp, S, rs.rand(n['t'], ranks['t']) + 0.1


def make_plan(dt, eng, n, ranks, rels, thetas, model):
    """rels: [(i, j, R or DeviceMatrix)]; thetas: [] or [('t', constraint)]."""
    Gp, S, G0 = model
    types = ['t'] + sorted(o for o in n if o != 't')
    plan = DevicePlan(types, n, ranks, [(i, j, R, None) for i, j, R in rels], thetas, nat.SKF_TRANSFORM, dtype=dt,
                      target='t', engine=eng)
    for o in types[1:]:
        plan.set_factor(o, Gp[o])
    plan.set_factor('t', G0)
    for k, s in enumerate(S):
        plan.set_backbone(k, s)
    return plan


def contraction_bytes(dt, n, ranks, rel_list):
    """Relation bytes the contractions of prepare_transform read as stored, by the form the engine keeps each relation
    in (skf_plan_get_profile): the one place a test observes which form ran.  bf16: 0 / 1 relations as lists over bf16
    factor rows (4 bytes per one) when both ranks allow the gathers and at most one entry in 80 is set, else as a bitmap
    (1 bit per entry); any other relation as stored (2 bytes bf16, 4 f32, 8 f64 per entry).  Also returns the forms."""
    total, forms = 0.0, []
    for i, j, R in rel_list:
        cells, nnz = R.size, int(np.count_nonzero(R))
        binary = dt == 'bf16' and bool(np.all((R == 0) | (R == 1)))
        if binary and ranks[i] in GATHER_RANKS and ranks[j] in GATHER_RANKS and nnz <= max(cells // GATHER_PER, 1):
            forms.append('gathers')
            total += 4.0 * nnz
        elif binary:
            assert nnz > cells // 256, 'a 0 / 1 relation this sparse takes the f32 row gathers, which the model does not hold'
            forms.append('bitmap')
            total += cells / 8.0
        else:
            forms.append('dense')
            total += cells * {'bf16': 2.0, 'f32': 4.0, 'f64': 8.0}[dt]
    return total, forms


def read_contractions(plan, rel_list):
    """The device's P (target row) / Q (target column) of every relation: the one a fold-in plan keeps."""
    return [plan.get_contraction(k, 0 if i == 't' else 1).astype(np.float64) for k, (i, j, _) in enumerate(rel_list)]


# ---- the host model ---------------------------------------------------------------------------------------------------
class FoldModel(object):
    def __init__(self, dtype, n, ranks, rels, theta):
        self.dtype, self.n, self.c = dtype, n, ranks
        self.u, self.um = U_ACC[dtype], U_M[dtype]
        self.mt = 'f64' if dtype == 'f64' else 'f32'
        self.rels = rels
        self.work = [store_round(R, dtype) for _, _, R in rels]        # the relation as the engine stores it
        self.theta = theta
        nz = 0 if theta is None else int(np.count_nonzero(theta))       # (CSR up to n * n / the library's divisor)
        self.theta_sparse = 0 < nz <= n['t'] * n['t'] // small_graph_limits()['constraint_nnz_divisor']

    def operand(self, G):
        return store_round(G, 'bf16') if self.dtype == 'bf16' else G          # (bf16 G^T / bf16 factor rows)

    def contractions(self, Gp, X):
        n, u, um = self.n, self.u, self.um
        res = {}
        for k, (i, j, _) in enumerate(self.rels):
            r = self.work[k]
            if i == 't':
                G = self.operand(Gp[j])
                h = r @ G
                b = (n[j] + 10) * u * (np.abs(r) @ np.abs(G)) + um * np.abs(h)
                res['rel %d (t x %s) contraction P = R G_j' % (k, j)] = ratio(X[k] - h, b)
            else:
                G = self.operand(Gp[i])
                h = r.T @ G
                b = (n[i] + 10) * u * (np.abs(r).T @ np.abs(G)) + um * np.abs(h)
                res['rel %d (%s x t) contraction Q = R^T G_i' % (k, i)] = ratio(X[k] - h, b)
        return res

    def prepared(self, Gp, S, X):
        """Ec, Dc and the B sums of prepare_transform from the device's P / Q, with their bounds."""
        n, c, u, um = self.n, self.c, self.u, self.um
        ct = c['t']
        pr = {'Ec': np.zeros((n['t'], ct)), 'Dc': np.zeros((n['t'], ct)), 'bC': np.zeros((n['t'], ct)),
              'Bn': np.zeros((ct, ct)), 'Bp': np.zeros((ct, ct)), 'bB': np.zeros((ct, ct))}
        for k, (i, j, _) in enumerate(self.rels):
            s = S[k]
            if i == 't':                                                   # _dfmf.py:392-405
                o = j
                A = X[k] @ s.T
                bA = (c[o] + 2) * u * (np.abs(X[k]) @ np.abs(s).T)
                gram = Gp[o].T @ Gp[o]
                B = s @ gram @ s.T
                bB = (c[o] + n[o] + 4) * U64 * (np.abs(s) @ np.abs(gram) @ np.abs(s).T)
            else:                                                          # _dfmf.py:407-419
                o = i
                A = X[k] @ s
                bA = (c[o] + 2) * u * (np.abs(X[k]) @ np.abs(s))
                gram = Gp[o].T @ Gp[o]
                B = s.T @ gram @ s
                bB = (c[o] + n[o] + 4) * U64 * (np.abs(s).T @ np.abs(gram) @ np.abs(s))
            pr['Ec'] += pos(A)
            pr['Dc'] += neg(A)
            pr['bC'] += bA + um * np.abs(A)
            pr['Bn'] += neg(B)
            pr['Bp'] += pos(B)
            pr['bB'] += bB
        return pr

    def step(self, pr, G0, G1):
        """worst |delta| / bound of the device's G1 against the update of G0 (the device's previous factor)."""
        u, um, ct = self.u, self.um, self.c['t']
        E, D, bE = pr['Ec'].copy(), pr['Dc'].copy(), pr['bC'].copy()
        Bn, Bp = pr['Bn'], pr['Bp']
        Bnm, Bpm = store_round(Bn, self.mt), store_round(Bp, self.mt)          # (e): staged in the master type
        GB = G0 @ Bnm
        E += GB
        D += G0 @ Bpm
        bE += (ct + 2) * u * (np.abs(G0) @ (Bnm + Bpm)) + np.abs(G0) @ (pr['bB'] + um * (Bn + Bp)) + um * np.abs(GB)
        nterms = 2 * len(self.rels) + 2
        th = self.theta
        if th is not None:
            if self.dtype == 'bf16' and not self.theta_sparse:              # bf16 halves against the stored bf16 G^T
                tp, tn, Gt = store_round(pos(th), 'bf16'), store_round(neg(th), 'bf16'), store_round(G0, 'bf16')
            else:
                tm = store_round(th, self.mt)
                tp, tn, Gt = pos(tm), neg(tm), G0
            k_acc = (np.count_nonzero(th, axis=1)[:, None] if self.theta_sparse else self.n['t']) + 10
            D += tp @ Gt
            E += tn @ Gt
            bE += k_acc * u * (np.abs(th) @ np.abs(Gt)) + um * (np.abs(th) @ np.abs(Gt))
            nterms += 2
        Dm = np.maximum(D, EPS)
        Gh = G0 * np.sqrt(E / Dm)
        bEt = bE + nterms * um * E
        bDt = bE + nterms * um * D
        rel = 0.5 * (np.where(bEt == 0, 0.0, bEt / np.maximum(E, 1e-300)) + bDt / Dm) + 3 * um
        return ratio(G1 - Gh, Gh * rel)

    def sqerr(self, Gt, Gp, S, got):
        """relation_sqerr of every relation against the f64 host sum over the engine's stored relation."""
        n, u = self.n, self.u
        dm = DenseModel(self.dtype, nat.SKF_DFMF, n, self.c, [], [], [])
        res = {}
        for k, (i, j, _) in enumerate(self.rels):
            Gi, Gj = (Gt if i == 't' else Gp[i]), (Gt if j == 't' else Gp[j])
            X, eX = dm.completion(Gi, S[k], Gj, rounded=False)
            e = self.work[k] - X
            sq = np.sum(e ** 2)
            b = np.sum(2 * np.abs(e) * eX + eX ** 2) + (n[i] + n[j] + 10) * max(u, U64) * sq
            res['rel %d (%s x %s) relation_sqerr' % (k, i, j)] = abs(got[k] - sq) / (K_SAFE * b)
        return res


def graph_of(n_t, c_t, partners):
    n, ranks = {'t': n_t}, {'t': c_t}
    for o, (no, co) in partners.items():
        n[o], ranks[o] = no, co
    return n, ranks


def report(res, what):
    out = {}
    for k, v in res.items():
        name = '%s: %s' % (what, k)
        out[name] = within(v, 1.0, '%s, |delta| / model bound' % name)
    return out


# ---- one fold-in, stage by stage ---------------------------------------------------------------------------------------
def fold_case(engine, n_t, c_t, partners, rels, theta, kernel, what, iters=3, seed=0):
    """partners: {type: (objects, rank)}.  Runs `iters` (>= 3) single iterations, the k = 2 / 3 repeats and the two
    re-preparations, and holds each to the host model (module comment).  Returns {check: worst |delta| / bound}."""
    assert iters >= 3
    dt, eng = ENGINES[engine]
    n, ranks = graph_of(n_t, c_t, partners)
    assert kernel_of(engine, n_t, c_t, theta) == kernel, 'case does not take the %s iteration' % kernel
    rs = np.random.RandomState(seed)
    rel_list, th = fold_graph(n, rels, theta, rs)
    model = frozen_model(dt, n, ranks, rel_list, rs)
    S = model[1]
    S2 = list(S)
    S2[0] = store_round(rs.rand(*S[0].shape) * 2.0 - 1.0, 'f64' if dt == 'f64' else 'f32')
    moved = rel_list[0][1] if rel_list[0][0] == 't' else rel_list[0][0]      # the partner whose factor is set anew
    Gnew = rs.rand(n[moved], ranks[moved]) + 0.2
    plan = make_plan(dt, eng, n, ranks, rel_list, [('t', th)] if th is not None else [], model)
    try:
        assert plan.batchable() == (kernel != 'generic'), 'case does not take the %s iteration' % kernel
        Gp = {o: plan.get_factor(o) for o in partners}
        G = [plan.get_factor('t')]
        plan.set_profiling(True)
        for it in range(iters):
            plan.iterate(1)
            G.append(plan.get_factor('t'))
            if it == 0:                       # the first iteration prepares: each relation contracted once, in its form
                want, forms = contraction_bytes(dt, n, ranks, rel_list)
                got = plan.get_profile()[3]
                assert got == want, '%s: relation forms %s read %r bytes, not %r' % (what, forms, got, want)
                plan.set_profiling(False)
        X = read_contractions(plan, rel_list)
        sq = [plan.relation_sqerr(k) for k in range(len(rel_list))]
        for k in (2, 3):                      # k iterations in one call: the bits of k single ones (G / Galt swaps)
            plan.set_factor('t', G[0])
            plan.iterate(k)
            np.testing.assert_array_equal(plan.get_factor('t'), G[k], err_msg='%s: iterate(%d) vs %d x iterate(1)' % (what, k, k))
        plan.set_backbone(0, S2[0])           # re-preparation: a new backbone ...
        plan.iterate(1)
        Gb = plan.get_factor('t')
        plan.set_factor(moved, Gnew)          # ... and a new partner factor
        Gp2 = dict(Gp)
        Gp2[moved] = plan.get_factor(moved)
        plan.iterate(1)
        Gc = plan.get_factor('t')
        X2 = read_contractions(plan, rel_list)
    finally:
        plan.close()
    host = FoldModel(dt, n, ranks, rel_list, th)
    res = host.contractions(Gp, X)
    pr = host.prepared(Gp, S, X)
    for it in range(iters):
        res['it %d: update G1 = G0 o sqrt(E / D), per element' % (it + 1)] = host.step(pr, G[it], G[it + 1])
    res.update(host.sqerr(G[iters], Gp, S, sq))
    res['after set_backbone: update'] = host.step(host.prepared(Gp, S2, X), G[3], Gb)
    for k, v in host.contractions(Gp2, X2).items():
        res['after set_factor: ' + k] = v
    res['after set_factor: update'] = host.step(host.prepared(Gp2, S2, X2), Gb, Gc)
    return report(res, what)


# ---- fold-ins into several models in shared launches (skf_iterate_batch, fold_steps) -------------------------------------
def batch_case(engine, n_plans, n_t, c_t, partners, rels, what, seed=0):
    """`n_plans` plans over ONE set of uploaded relations, each with its own frozen model and G0: every plan iterated
    alone (three steps, each held to the plan's own host model), then all of them batched -- an even (2) and an odd (1)
    iteration count -- must give the bits of the plan alone.  Refusals: 65 plans (SKF_E_INVALID) and a batch holding a
    plan with a target constraint (False, nothing launched).  Returns {check: worst |delta| / bound}."""
    dt, eng = ENGINES[engine]
    n, ranks = graph_of(n_t, c_t, partners)
    assert kernel_of(engine, n_t, c_t, None) != 'generic'
    rs = np.random.RandomState(seed)
    rel_list, th = fold_graph(n, rels, 'csr', rs)
    up, up_th = upload_graph([(i, j, R, None) for i, j, R in rel_list], [('t', th)], dt)
    up = [(i, j, d) for i, j, d, _ in up]
    models = [frozen_model(dt, n, ranks, rel_list, rs) for _ in range(n_plans)]
    host = FoldModel(dt, n, ranks, rel_list, None)
    plans, res = [], {}
    try:
        for m in models:
            plans.append(make_plan(dt, eng, n, ranks, up, [], m))
        alone = []
        for q, plan in enumerate(plans):
            assert plan.batchable(), 'case does not take the fused fold-in'
            Gp = {o: plan.get_factor(o) for o in partners}
            G = [plan.get_factor('t')]
            for _ in range(3):
                plan.iterate(1)
                G.append(plan.get_factor('t'))
            pr = host.prepared(Gp, models[q][1], read_contractions(plan, rel_list))
            res['plan %d: update, worst of 3 iterations' % q] = max(host.step(pr, G[it], G[it + 1]) for it in range(3))
            alone.append(G)
            plan.set_factor('t', G[0])
        assert DevicePlan.iterate_batch(plans, 2)
        for q, plan in enumerate(plans):
            np.testing.assert_array_equal(plan.get_factor('t'), alone[q][2], err_msg='%s: plan %d, 2 batched iterations' % (what, q))
        assert DevicePlan.iterate_batch(plans, 1)
        for q, plan in enumerate(plans):
            np.testing.assert_array_equal(plan.get_factor('t'), alone[q][3], err_msg='%s: plan %d, 2 + 1 batched iterations' % (what, q))
        other = make_plan(dt, eng, n, ranks, up, up_th, models[0])         # a target constraint: the generic path
        plans.append(other)
        assert not other.batchable()
        before = plans[0].get_factor('t')
        assert DevicePlan.iterate_batch([plans[0], other], 1) is False
        np.testing.assert_array_equal(plans[0].get_factor('t'), before)
        many = plans if len(plans) == 65 else (plans * 65)[:65]           # (distinct plans when there are 64 + 1)
        with pytest.raises(nat.SkfNativeError, match=r'1 \.\. 64 plans') as exc:
            DevicePlan.iterate_batch(many, 1)
        assert exc.value.code == nat.SKF_E_INVALID
    finally:
        for plan in plans:
            plan.close()
    return report(res, what)


# ---- the cases (tests/test_emul_engine.py runs EMUL and EMUL_BATCH, tests/test_gpu_foldin_model.py GPU and BATCH) --------
# name: (engine, n_t, c_t, partners {type: (objects, rank)}, relations [(target side, partner, kind)], target
# constraint, kernel)
EMUL = {
    # f64 <2,2,16>: both sides, the row-side pair given twice, c_t % 16 != 0
    'fused_f64_big': ('f64', 65, 66, {'a': (70, 9), 'b': (40, 20)},
                      [('row', 'a', 'neg'), ('row', 'a', 'pos'), ('col', 'b', 'neg')], None, 'f64<2,2,16>'),
    # f64 <1,1,16>: a rank-1 partner, the column-side pair twice
    'fused_f64_small': ('f64', 33, 17, {'a': (50, 5), 'b': (31, 1)},
                        [('row', 'a', 'neg'), ('col', 'b', 'pos'), ('col', 'b', 'neg')], None, 'f64<1,1,16>'),
    # f32: one new object of rank 1 -- both strides of Bn / Bp are 1 (the k-fast LDS store)
    'fused_f32_one': ('f32', 1, 1, {'a': (40, 3), 'b': (23, 2)},
                      [('row', 'a', 'neg'), ('col', 'b', 'neg')], None, 'f32<1,1,16>'),
    # bf16: row gathers (ranks 64 / 128) on the column side, a bitmap and a real-valued relation on the row side
    'fused_bf16': ('bf16', 65, 64, {'a': (90, 128), 'b': (70, 5)},
                   [('col', 'a', 'sparse_ones'), ('row', 'b', 'ones'), ('row', 'b', 'neg')], None, 'f32<1,1,16>'),
    # the generic path: a dense constraint (f64), a CSR constraint (f32), a dense constraint in bf16 (G^T refresh), VALU
    'generic_f64_dense': ('f64', 33, 5, {'a': (40, 7)}, [('col', 'a', 'neg'), ('row', 'a', 'pos')], 'dense', 'generic'),
    'generic_f32_csr': ('f32', 65, 17, {'a': (50, 6)}, [('row', 'a', 'neg'), ('col', 'a', 'neg')], 'csr', 'generic'),
    'generic_bf16_dense': ('bf16', 40, 8, {'a': (50, 6), 'b': (30, 4)},
                           [('row', 'a', 'neg'), ('col', 'b', 'ones')], 'dense', 'generic'),
    'valu_f32': ('f32_valu', 33, 17, {'a': (40, 5)}, [('row', 'a', 'neg'), ('col', 'a', 'pos')], None, 'generic'),
}
# name: (engine, plans, n_t, c_t, partners, relations)
EMUL_BATCH = {
    # 17 plans: the second launch chunk (plans 16 ..) of fold_steps
    'batch17_f64': ('f64', 17, 33, 5, {'a': (30, 4), 'b': (20, 3)}, [('row', 'a', 'neg'), ('col', 'b', 'neg')]),
}

# GPU: the cases above and every instantiation at object counts 1 .. 4099 and target ranks 1 .. 320, both relation kinds
# and sides, both constraint forms in every engine and the VALU engine in f32 and f64
GPU = dict(EMUL)
GPU.update({
    'fused_f64_big_4099': ('f64', 4099, 128, {'a': (301, 65), 'b': (257, 16)},
                           [('row', 'a', 'neg'), ('col', 'b', 'neg'), ('col', 'b', 'pos')], None, 'f64<2,2,16>'),
    'fused_f64_big_320': ('f64', 257, 320, {'a': (129, 17), 'b': (65, 64)},
                          [('row', 'a', 'neg'), ('row', 'a', 'pos'), ('col', 'b', 'neg')], None, 'f64<2,2,16>'),
    'fused_f64_n64_c128': ('f64', 64, 128, {'a': (100, 5)}, [('row', 'a', 'neg'), ('col', 'a', 'neg')], None, 'f64<1,1,16>'),
    'fused_f64_n65_c64': ('f64', 65, 64, {'a': (100, 17)}, [('col', 'a', 'neg'), ('row', 'a', 'pos')], None, 'f64<1,1,16>'),
    'fused_f64_one': ('f64', 1, 1, {'a': (40, 3)}, [('row', 'a', 'neg'), ('col', 'a', 'neg')], None, 'f64<1,1,16>'),
    'fused_f32_257_65': ('f32', 257, 65, {'a': (301, 128), 'b': (33, 5)},
                         [('row', 'a', 'neg'), ('col', 'b', 'pos'), ('col', 'b', 'neg')], None, 'f32<1,1,16>'),
    'fused_f32_4099_320': ('f32', 4099, 320, {'a': (257, 17)}, [('row', 'a', 'neg'), ('col', 'a', 'neg')], None,
                           'f32<1,1,16>'),
    'fused_bf16_4099_128': ('bf16', 4099, 128, {'a': (301, 64), 'b': (129, 16)},
                            [('row', 'a', 'sparse_ones'), ('col', 'a', 'ones'), ('col', 'b', 'neg'), ('row', 'b', 'pos')],
                            None, 'f32<1,1,16>'),
    'fused_bf16_33_5': ('bf16', 33, 5, {'a': (129, 64), 'b': (40, 7)}, [('row', 'a', 'ones'), ('col', 'b', 'neg')], None,
                        'f32<1,1,16>'),
    'generic_f64_csr': ('f64', 257, 16, {'a': (129, 9)}, [('row', 'a', 'neg'), ('col', 'a', 'neg')], 'csr', 'generic'),
    'generic_f32_dense': ('f32', 64, 65, {'a': (100, 8)}, [('col', 'a', 'neg'), ('row', 'a', 'pos')], 'dense', 'generic'),
    'generic_bf16_csr': ('bf16', 257, 17, {'a': (129, 64), 'b': (65, 8)},
                         [('row', 'a', 'sparse_ones'), ('col', 'b', 'neg')], 'csr', 'generic'),
    'valu_f64': ('f64_valu', 65, 66, {'a': (70, 9)}, [('row', 'a', 'neg'), ('col', 'a', 'neg')], None, 'generic'),
})
BATCH = dict(EMUL_BATCH)
BATCH.update({
    'batch1_f64': ('f64', 1, 65, 66, {'a': (70, 9)}, [('row', 'a', 'neg'), ('col', 'a', 'neg')]),
    'batch2_f32': ('f32', 2, 33, 5, {'a': (30, 4)}, [('row', 'a', 'neg'), ('col', 'a', 'pos')]),
    'batch16_bf16': ('bf16', 16, 40, 17, {'a': (50, 6)}, [('row', 'a', 'ones'), ('col', 'a', 'neg')]),
    'batch33_f32': ('f32', 33, 65, 17, {'a': (40, 5), 'b': (20, 3)}, [('row', 'a', 'neg'), ('col', 'b', 'neg')]),
    'batch64_f64': ('f64', 64, 33, 5, {'a': (30, 4), 'b': (20, 3)}, [('row', 'a', 'neg'), ('col', 'b', 'neg')]),
})
