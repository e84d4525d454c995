"""One dense iteration of a plan held to a host model, stage by stage (the sibling of known_cases.py, which does the same
for the known-entry lists).  The same cases run on the host emulator (tests/test_emul_engine.py, `dense`) and on the GPU
(tests/test_gpu_dense_model.py).  Every stage is checked on the DEVICE's own inputs to that stage, so that a failure points
at one kernel family:

  1. contractions  P = R G_j, Q = R^T G_i (relation_gemm / bitmap / row gathers; DFMC: of the completed relation)
  2. backbone      S = K_i W K_j, W in the device's own form (G_i^T P or Q^T G_j), K = pinv(G^T G) of the device's G0
  3. update        G1 = G0 o sqrt(E / max(D, eps)), E and D formed on the host from the device's P, Q, S, the f64 Gram
                   matrices of G0 and the constraints (side_update_kernel, the EPI_SPLIT_* epilogues, the Theta split,
                   theta_spmm_kernel, mult_update_kernel / mult_update_transpose_kernel, the three small-graph launches)
  4. completion    DFMC, dense path: P and Q above are contractions of R_c = R on the known entries and (G0_i S1 G0_j^T)
                   on the unknown ones (EPI_MASKED_STORE; bf16: EPI_T_COMPLETE in its list and blend forms), and
                   relation_sqerr of the working copy against the host's completed relation
  5. G^T refresh   bf16: a second iteration, whose contractions read bf16(G1) of the G1 the device returned

Error model.  The host repeats the engine's operand roundings and nothing else -- f64: none; f32: relation, factors,
constraints, P, Q, E, D in f32, S as its f32 rounding in the n-sized products; bf16: the one bf16 copy of R (0 / 1 relations
exact), bf16 G^T in the contractions and in dense Theta products (whose halves are bf16 too), f32 everywhere else -- and the
c x c algebra, the Gram matrices and W in f64 in every engine.  What remains is bounded element by element:
  (a) an accumulation of k products in unit u (2^-53 for f64, 2^-24 for f32 accumulation) moves an element by at most
      (k + 2) u (|X| |Y|) -- k = n_j (+ split-K partials, 8 at most) for P, n_i for Q, c_j for P S^T, c_i for Q S, c for
      G B, n (or the nonzeros of the row) for Theta G; every stored result adds u_m |value|;
  (b) the +- split is 1-Lipschitz: |d(A+)|, |d(A-)| <= |dA| -- an element of A near zero that flips sign moves at most its
      own error bound between E and D;
  (c) B = S Gram_j S^T and its sums are f64 from the f64 S; where the host holds S only as its f32 rounding (f32 / bf16
      engines) the host's B is off by up to 2 u32 |S| |Gram| |S|^T, plus the f32 rounding of the sums;
  (d) E and D are sums of non-negative terms, so  |dG1| / G1 <= 1/2 (|dE| / E + |dD| / D) + 3 u_m;
  (e) bf16 roundings of values the device computes itself (H = G_i S of the completion, the completed value) may fall
      either way where the value lies within its error band of a bf16 midpoint: the host takes the rounding of the value
      and carries `band` = the largest distance to the roundings of the band's two ends (0 almost everywhere) as an
      extra error of that operand, first order;
  (f) the backbone is the one stage gated norm-wise: a relative error e_W of W becomes up to kappa_i kappa_j e_W in S and
      the pseudo-inverses add kappa (n + c) u64 each (kappa = cond(G^T G) of the device's own G0 over
      its non-null part, so that a rank-deficient Gram takes the deflation route and stays gated).
Each bound is known_cases.K_SAFE times the first-order sum above; every check goes through helpers.within."""
import numpy as np
import scipy.linalg

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan
from helpers import within
from known_cases import K_SAFE, U_ACC, store_round

U64 = 2.0 ** -53
U_M = {'f64': 2.0 ** -53, 'f32': 2.0 ** -24, 'bf16': 2.0 ** -24}      # unit of the n-sized masters
SMALLC = 64                                                            # skf_api.hip: the small-chain / small-graph limit
EPS = 2.220446049250313e-16


def band(x, err, dtype):
    """x rounded as the engine stores it, and how far the device's rounding may lie from it when the device's x is
    anywhere in [x - err, x + err] (model (e))."""
    xr = store_round(x, dtype)
    d = np.maximum(np.abs(store_round(x + err, dtype) - xr), np.abs(xr - store_round(x - err, dtype)))
    return xr, d


def ratio(dev, bound):
    """worst |delta| / (K_SAFE bound); an element with a zero bound must match exactly."""
    dev = np.abs(dev)
    return float(np.max(np.where(dev == 0, 0.0, dev / np.maximum(K_SAFE * bound, 1e-300)))) if dev.size else 0.0


def pos(x):
    return np.maximum(x, 0.0)


def neg(x):
    return np.maximum(-x, 0.0)


def gram_condition(G):
    """cond(G^T G) over its non-null part (the cut-off of the oracle's pinv)."""
    w = np.linalg.eigvalsh(G.T @ G)
    keep = w > max(G.shape) * np.finfo(float).eps * w[-1]
    return float(w[-1] / w[keep][0])


# ---- cases -----------------------------------------------------------------------------------------------------------
def dfmc_mask(n_a, n_b, known, rs):
    """UNKNOWN pattern (True = unknown) with `known` of the entries known and the edges of the completion epilogue: a fully
    unknown row and column, a fully known row; rows with runs of known entries in an unknown row and runs of unknown
    entries in a known row that start and end on and off the 8-entry (16-byte bf16) chunks, the last ones at the last
    column."""
    M = rs.rand(n_a, n_b) >= known
    M[1, :] = True
    M[:, 2] = True
    M[3, :] = False
    runs = [(8, 16), (5, 19), (16, 17), (n_b - 9, n_b), (n_b - 8 - n_b % 8, n_b), (n_b - 1, n_b)]
    for k, (a, b) in enumerate(runs):
        M[4 + k, :] = True
        M[4 + k, max(a, 0):b] = False
        M[4 + len(runs) + k, :] = False
        M[4 + len(runs) + k, max(a, 0):b] = True
    return M


def relation(kind, n_a, n_b, rs):
    if kind == 'neg':                       # both signs: both sides of every +- split populated
        return rs.rand(n_a, n_b) * 2.0 - 0.6
    if kind == 'pos':
        return rs.rand(n_a, n_b)
    if kind == 'ones':                      # dense 0 / 1: a bitmap in the bf16 engine
        return (rs.rand(n_a, n_b) < 0.3).astype(np.float64)
    if kind == 'sparse_ones':               # at most one in 80: row / column gathers in the bf16 engine
        R = (rs.rand(n_a, n_b) < 0.008).astype(np.float64)
        R[0, -1] = R[-1, 0] = 1.0
        return R
    raise ValueError(kind)


def constraint(kind, n, rs):
    if kind == 'dense':                     # every entry set, both signs
        th = (rs.rand(n, n) - 0.7) * 0.02
        return th + th.T
    assert kind == 'csr'                    # a few entries per row, negative off-diagonals, a positive diagonal
    th = -0.02 * (rs.rand(n, n) < 1.0 / n) * rs.rand(n, n)      # (sparse: <= n^2 / 16 nonzeros)
    th = th + th.T
    np.fill_diagonal(th, 0.03)
    th[-1, :] = 0.0
    th[:, -1] = 0.0
    th[-1, -1] = 0.01
    th[-1, 0] = th[0, -1] = -0.015          # the last row: one entry besides the diagonal
    return th


def graph(n, ranks, rels, thetas, seed, deficient=None):
    """rels: [(row, col, kind, known share or None)], thetas: [(type, 'dense' | 'csr')]; deficient: a type whose G0 has
    two equal columns (a rank-deficient Gram)."""
    rs = np.random.RandomState(seed)
    out_rels = []
    for i, j, kind, known in rels:
        R = relation(kind, n[i], n[j], rs)
        out_rels.append((i, j, R, None if known is None else dfmc_mask(n[i], n[j], known, rs)))
    out_th = [(t, constraint(kind, n[t], rs)) for t, kind in thetas]
    G0 = {t: rs.rand(n[t], ranks[t]) + 0.1 for t in n}
    if deficient is not None and ranks[deficient] > 1:
        G0[deficient][:, -1] = G0[deficient][:, 0]
    return out_rels, out_th, G0


# ---- the schedule's choice of W (skf_schedule.inc iterate_fit_pipelined, skf_stages.inc stage_contract, skf_small.h) ---
def pipelines(variant, ranks, rels, thetas):
    """can_pipeline of skf_schedule.inc for the plans built here (MFMA engine, overlap on, no row blocks)."""
    if any(kind == 'dense' for _, kind in thetas) or not rels or len(rels) > 64:
        return False
    cmax = 256 if variant == nat.SKF_DFMC else 512
    if any(c > cmax for c in ranks.values()) or all(c <= SMALLC for c in ranks.values()):
        return False
    if variant == nat.SKF_DFMF and any(c <= SMALLC for c in ranks.values()):
        return False
    return not any(m is not None and variant != nat.SKF_DFMC for *_, m in rels)


def w_by_q(schedule, variant, n, ranks, rels):
    """[True where W = Q^T G_j] per relation, as the schedule that runs forms it: a masked DFMC relation through the
    narrower factor (c_i < c_j) in every schedule; in the pipeline an unmasked relation by Q when it is not the last
    of the cost order and 5 n_j <= 3 n_i; else G_i^T P (the small-graph schedule always)."""
    dfmc = variant == nat.SKF_DFMC
    out = [dfmc and m is not None and ranks[i] < ranks[j] for i, j, _, m in rels]
    if schedule == 'pipeline':
        cost = [n[i] * n[j] * (ranks[i] + ranks[j]) for i, j, _, _ in rels]
        order = sorted(range(len(rels)), key=lambda k: -cost[k])          # (stable, as std::stable_sort)
        for q, k in enumerate(order):
            i, j, _, m = rels[k]
            if not (dfmc and m is not None):
                out[k] = q + 1 < len(rels) and 5 * n[j] <= 3 * n[i]
    return out


# ---- the case ---------------------------------------------------------------------------------------------------------
SCHEDULE_ENV = {'pipeline': {}, 'staged': {'SKF_NO_PIPELINE': '1'}, 'small': {}, 'chain': {'SKF_NO_SMALL_FUSED': '1'}}


def dense_case(dtype, schedule, n, ranks, rels, thetas, what, monkeypatch, variant=nat.SKF_DFMF, iters=1, seed=0,
               deficient=None):
    """Builds the graph, runs `iters` single iterations on the engine `dtype` under `schedule` and holds each to the
    host model (module comment).  Returns {check: worst |delta| / bound}."""
    for k, v in SCHEDULE_ENV[schedule].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('SKF_DFMC_SPARSE', '0')
    types = list(n)
    rel_list, th_list, G0 = graph(n, ranks, rels, thetas, seed, deficient)
    if schedule == 'pipeline':
        assert pipelines(variant, ranks, rel_list, thetas), 'case does not take the relation pipeline'
    byq = w_by_q(schedule, variant, n, ranks, rel_list)
    plan = DevicePlan(types, n, ranks, rel_list, th_list, variant, dtype=dtype, sparse_known=False)
    snaps = []
    try:
        assert plan.batchable() == (schedule == 'small'), 'case does not take the %s schedule' % schedule
        for t in types:
            plan.set_factor(t, G0[t])
        G = {t: plan.get_factor(t) for t in types}
        for _ in range(iters):
            plan.iterate(1)
            snap = {'G0': G,
                    'S': [plan.get_backbone(k) for k in range(len(rel_list))],
                    'P': [plan.get_contraction(k, 0).astype(np.float64) for k in range(len(rel_list))],
                    'Q': [plan.get_contraction(k, 1).astype(np.float64) for k in range(len(rel_list))]}
            G = {t: plan.get_factor(t) for t in types}
            assert all(np.isfinite(G[t]).all() for t in types), '%s: non-finite factor' % what
            snap['G1'] = G
            snap['sq'] = [plan.relation_sqerr(k) if m is not None else None for k, (_, _, _, m) in enumerate(rel_list)]
            snaps.append(snap)
    finally:
        plan.close()
    model = Model(dtype, variant, n, ranks, rel_list, th_list, byq)
    out = {}
    for it, snap in enumerate(snaps):
        for k, v in model.iteration(snap).items():
            name = '%s it %d: %s' % (what, it + 1, k)
            out[name] = within(v, 1.0, '%s, |delta| / model bound' % name)
    return out


class Model(object):
    """The host side of dense_case: the relations' working copies (value and band) carried from iteration to iteration."""

    def __init__(self, dtype, variant, n, ranks, rels, thetas, byq):
        self.dtype, self.variant, self.n, self.ranks, self.byq = dtype, variant, n, ranks, byq
        self.u, self.um = U_ACC[dtype], U_M[dtype]
        self.rels, self.thetas = rels, thetas
        self.work = []
        for i, j, R, M in rels:
            r = store_round(R, dtype)
            if M is not None:
                r = np.where(M, 0.0, r)              # iteration 1 reads the unknown entries as 0 (_dfmc.py:287-292)
            self.work.append((r, np.zeros_like(r)))

    def contraction_operand(self, G):
        return store_round(G, 'bf16') if self.dtype == 'bf16' else G       # (the stored bf16 G^T)

    def completion(self, Gi, S, Gj, rounded=True):
        """G_i S G_j^T as the engine forms the completed entries (rounded=False: the f32 value before the store, as the
        squared-error pass uses it), and its error bound: f64 / f32 -- a plain bound; bf16 -- the band of model (e),
        H = G_i S rounded to bf16 and, when `rounded`, the value too."""
        dt, u = self.dtype, self.u
        ci, cj = Gi.shape[1], Gj.shape[1]
        H = Gi @ S
        eH = (ci + 2) * u * (np.abs(Gi) @ np.abs(S)) + (u * np.abs(Gi) @ np.abs(S) if dt != 'f64' else 0.0)
        if dt != 'bf16':
            v = H @ Gj.T
            err = (cj + 2) * u * (np.abs(H) @ np.abs(Gj).T) + eH @ np.abs(Gj).T + self.um * np.abs(v)
            return store_round(v, dt), err
        Hb, dH = band(H, eH + self.um * np.abs(H), 'bf16')
        Gb = store_round(Gj, 'bf16')
        v = Hb @ Gb.T
        err = (cj + 2) * u * (np.abs(Hb) @ np.abs(Gb).T) + dH @ np.abs(Gb).T
        return band(v, err, 'bf16') if rounded else (v, err)

    def iteration(self, s):
        dt, u, um, n, c = self.dtype, self.u, self.um, self.n, self.ranks
        G0, G1 = s['G0'], s['G1']
        Gc = {t: self.contraction_operand(G0[t]) for t in G0}
        gram = {t: G0[t].T @ G0[t] for t in G0}
        kap = {t: gram_condition(G0[t]) for t in G0}
        res = {}
        E = {t: np.zeros_like(G0[t]) for t in G0}
        D = {t: np.zeros_like(G0[t]) for t in G0}
        bE = {t: np.zeros_like(G0[t]) for t in G0}           # bounds of |dE|, |dD| (they share them: model (b))
        Bn = {t: np.zeros((c[t], c[t])) for t in G0}
        Bp = {t: np.zeros((c[t], c[t])) for t in G0}
        bB = {t: np.zeros((c[t], c[t])) for t in G0}
        for k, (i, j, R, M) in enumerate(self.rels):
            S, P, Q = s['S'][k], s['P'][k], s['Q'][k]
            r, dr = self.work[k]
            tag = 'rel %d (%s x %s)' % (k, i, j)
            # -- backbone: W in the device's form; a masked relation is contracted BEFORE its completion (host P / Q)
            Gi, Gj = G0[i], G0[j]
            if M is not None:
                Pw = r @ Gc[j]
                eP = (n[j] + 10) * u * (np.abs(r) @ np.abs(Gc[j])) + dr @ np.abs(Gc[j]) + um * np.abs(Pw)
                Qw = r.T @ Gc[i]
                eQ = (n[i] + 10) * u * (np.abs(r).T @ np.abs(Gc[i])) + dr.T @ np.abs(Gc[i]) + um * np.abs(Qw)
            else:
                Pw, eP, Qw, eQ = P, np.zeros_like(P), Q, np.zeros_like(Q)
            if self.byq[k]:
                W = Qw.T @ Gj
                eW = np.abs(eQ).T @ np.abs(Gj) + (n[j] + 2) * U64 * (np.abs(Qw).T @ np.abs(Gj))
            else:
                W = Gi.T @ Pw
                eW = np.abs(Gi).T @ np.abs(eP) + (n[i] + 2) * U64 * (np.abs(Gi).T @ np.abs(Pw))
            Ki, Kj = scipy.linalg.pinv(gram[i]), scipy.linalg.pinv(gram[j])
            Sh = Ki @ W @ Kj
            rel_S = np.linalg.norm(S - Sh) / np.linalg.norm(Sh)
            gate = (kap[i] * kap[j] * np.linalg.norm(eW) / np.linalg.norm(W) + (kap[i] * (n[i] + c[i]) + kap[j] * (n[j] + c[j])) * U64
                    + (um if dt != 'f64' else 0.0))
            res['%s backbone S (norm-wise, kappa %.0f x %.0f)' % (tag, kap[i], kap[j])] = rel_S / (K_SAFE * gate)
            # -- completion (DFMC): the working copy the contractions of this iteration read
            if M is not None and self.variant == nat.SKF_DFMC:
                vc, ec = self.completion(Gi, S, Gj)
                r = np.where(M, vc, r)
                dr = np.where(M, ec, 0.0)
                self.work[k] = (r, dr)
            # -- contractions
            Ph = r @ Gc[j]
            bP = (n[j] + 10) * u * (np.abs(r) @ np.abs(Gc[j])) + dr @ np.abs(Gc[j]) + um * np.abs(Ph)
            res['%s contraction P = R G_j' % tag] = ratio(P - Ph, bP)
            Qh = r.T @ Gc[i]
            bQ = (n[i] + 10) * u * (np.abs(r).T @ np.abs(Gc[i])) + dr.T @ np.abs(Gc[i]) + um * np.abs(Qh)
            res['%s contraction Q = R^T G_i' % tag] = ratio(Q - Qh, bQ)
            # -- the relation's E / D terms from the device's P, Q, S (S as the n-sized products read it)
            A = P @ S.T
            bA = (c[j] + 2) * u * (np.abs(P) @ np.abs(S).T)
            E[i] += pos(A)
            D[i] += neg(A)
            bE[i] += bA + um * np.abs(A)
            A = Q @ S
            bA = (c[i] + 2) * u * (np.abs(Q) @ np.abs(S))
            E[j] += pos(A)
            D[j] += neg(A)
            bE[j] += bA + um * np.abs(A)
            dS = 2 * um if dt != 'f64' else 0.0
            B = S @ gram[j] @ S.T
            Bn[i] += neg(B)
            Bp[i] += pos(B)
            bB[i] += ((c[j] + n[j] + 4) * U64 + dS) * (np.abs(S) @ np.abs(gram[j]) @ np.abs(S).T)
            B = S.T @ gram[i] @ S
            Bn[j] += neg(B)
            Bp[j] += pos(B)
            bB[j] += ((c[i] + n[i] + 4) * U64 + dS) * (np.abs(S).T @ np.abs(gram[i]) @ np.abs(S))
            # -- relation_sqerr of the working copy (DFMC): sum (R_c - G1_i S G1_j^T)^2
            if s['sq'][k] is not None:
                X, eX = self.completion(G1[i], S, G1[j], rounded=False)
                e = r - X
                sq = np.sum(e ** 2)
                b = np.sum(2 * np.abs(e) * (eX + dr) + (eX + dr) ** 2) + (n[j] + 10) * max(u, U64) * sq
                res['%s relation_sqerr of the completed working copy' % tag] = abs(s['sq'][k] - sq) / (K_SAFE * b)
        for t in G0:
            # -- type terms G B-+ (the B sums in f64, rounded to the master type)
            Bnm, Bpm = store_round(Bn[t], 'f32' if dt != 'f64' else 'f64'), store_round(Bp[t], 'f32' if dt != 'f64' else 'f64')
            GB = G0[t] @ Bnm
            E[t] += GB
            bE[t] += (c[t] + 2) * u * (np.abs(G0[t]) @ (Bnm + Bpm)) + np.abs(G0[t]) @ (bB[t] + um * (Bn[t] + Bp[t])) + um * np.abs(GB)
            D[t] += G0[t] @ Bpm
        for t, th in self.thetas:
            kind = 'csr' if np.count_nonzero(th) <= th.size // 4 else 'dense'
            if dt == 'bf16' and kind == 'dense':         # bf16 halves against the stored bf16 G^T
                tp, tn, Gt = store_round(pos(th), 'bf16'), store_round(neg(th), 'bf16'), Gc[t]
            else:
                tm = store_round(th, 'f32' if dt != 'f64' else 'f64')
                tp, tn, Gt = pos(tm), neg(tm), G0[t]
            k_acc = (np.count_nonzero(th, axis=1)[:, None] if kind == 'csr' else n[t]) + 10
            D[t] += tp @ Gt
            E[t] += tn @ Gt
            bE[t] += k_acc * u * (np.abs(th) @ np.abs(Gt)) + um * (np.abs(th) @ np.abs(Gt))
        for t in G0:
            Dm = np.maximum(D[t], EPS)
            Gh = G0[t] * np.sqrt(E[t] / Dm)
            nterms = 2 * len(self.rels) + 2 * len(self.thetas) + 2
            bEt = bE[t] + nterms * um * E[t]
            bDt = bE[t] + nterms * um * D[t]
            rel = 0.5 * (np.where(bEt == 0, 0.0, bEt / np.maximum(E[t], 1e-300)) + bDt / Dm) + 3 * um
            res['type %s update G1 = G0 o sqrt(E / D), per element' % t] = ratio(G1[t] - Gh, Gh * rel)
        return res


# ---- the cases (tests/test_emul_engine.py runs EMUL, tests/test_gpu_dense_model.py runs GPU) ------------------------------
# name: (engine, schedule, object counts, ranks, relations, constraints, keywords of dense_case)
DFMC = {'variant': nat.SKF_DFMC}
EMUL = {
    # relation pipeline, three relations into every type (the B sums accumulate: EPI_SPLIT_ACC), a bitmap and a 1-in-125
    # 0 / 1 relation (row / column gathers over 128-wide bf16 rows), a CSR constraint, the G^T refresh of iteration 2
    'pipeline_bf16': ('bf16', 'pipeline', {'a': 301, 'b': 129, 'c': 257}, {'a': 128, 'b': 65, 'c': 128},
                      [('a', 'b', 'neg', None), ('b', 'c', 'ones', None), ('a', 'c', 'sparse_ones', None)], [('b', 'csr')],
                      {'iters': 2}),
    'pipeline_f64': ('f64', 'pipeline', {'a': 129, 'b': 257, 'c': 301}, {'a': 65, 'b': 128, 'c': 66},
                     [('a', 'b', 'neg', None), ('b', 'c', 'neg', None), ('c', 'a', 'pos', None)], [('a', 'csr')], {}),
    # staged: a dense constraint (split while staged), a rank-deficient Gram, mixed ranks
    'staged_f32': ('f32', 'staged', {'a': 129, 'b': 63}, {'a': 65, 'b': 8},
                   [('a', 'b', 'neg', None), ('b', 'a', 'neg', None)], [('a', 'dense'), ('b', 'csr')], {'deficient': 'b'}),
    'staged_bf16': ('bf16', 'staged', {'a': 129, 'b': 63}, {'a': 65, 'b': 8},
                    [('a', 'b', 'neg', None), ('b', 'a', 'ones', None)], [('a', 'dense')], {'iters': 2}),
    # the three small-graph launches and the same graph on the staged schedule; one object, rank 1
    'small_f64': ('f64', 'small', {'a': 63, 'b': 65, 'c': 1}, {'a': 64, 'b': 1, 'c': 5},
                  [('a', 'b', 'neg', None), ('c', 'a', 'neg', None), ('b', 'c', 'pos', None)], [('a', 'csr')], {}),
    'chain_f32': ('f32', 'chain', {'a': 63, 'b': 65, 'c': 1}, {'a': 64, 'b': 1, 'c': 5},
                  [('a', 'b', 'neg', None), ('c', 'a', 'neg', None), ('b', 'c', 'pos', None)], [('a', 'csr')], {}),
    # DFMC dense path: the completion epilogue with per-tile lists (<= 1/8 known) and through the mask (above), masked store
    'dfmc_lists_bf16': ('bf16', 'staged', {'a': 263, 'b': 301}, {'a': 16, 'b': 8},
                        [('a', 'b', 'neg', 0.05), ('a', 'b', 'pos', None)], [('b', 'csr')], dict(DFMC, iters=2)),
    'dfmc_blend_bf16': ('bf16', 'pipeline', {'a': 263, 'b': 129}, {'a': 65, 'b': 16},
                        [('a', 'b', 'neg', 0.5)], [('a', 'csr')], dict(DFMC, iters=2)),
    'dfmc_f32': ('f32', 'staged', {'a': 129, 'b': 65}, {'a': 16, 'b': 8}, [('a', 'b', 'neg', 0.3)], [('a', 'csr')], DFMC),
}

# GPU: every case above in every engine whose plan takes it (the small-graph schedule has no bf16 engine), and relations
# of 4099 rows -- the 256-row LDS-DMA contraction and split-K by the time model inside a plan -- with ranks above 256
ENGINES = ('f64', 'f32', 'bf16')
BIG = {
    'big_pipeline': ('pipeline', {'a': 4099, 'b': 301, 'c': 257}, {'a': 128, 'b': 320, 'c': 256},
                     [('a', 'b', 'neg', None), ('b', 'c', 'ones', None), ('a', 'c', 'sparse_ones', None)], [('c', 'csr')],
                     {'iters': 2}),
    'big_staged': ('staged', {'a': 4099, 'b': 129}, {'a': 256, 'b': 64},
                   [('a', 'b', 'neg', None)], [('b', 'dense')], {'iters': 2}),
    'big_dfmc_lists': ('pipeline', {'a': 4099, 'b': 263}, {'a': 128, 'b': 64},
                       [('a', 'b', 'neg', 0.05)], [], dict(DFMC, iters=2)),
    'big_dfmc_blend': ('staged', {'a': 4099, 'b': 263}, {'a': 65, 'b': 256},
                       [('a', 'b', 'neg', 0.4)], [], dict(DFMC, iters=2)),
}


def gpu_cases():
    out = []
    for name, (_, sch, n, c, rels, ths, kw) in sorted(EMUL.items()):
        for dt in ENGINES:
            if sch == 'small' and dt == 'bf16':
                continue
            out.append(('%s/%s' % (name, dt), (dt, sch, n, c, rels, ths, dict(kw, iters=2))))
    for name, (sch, n, c, rels, ths, kw) in sorted(BIG.items()):
        for dt in ENGINES:
            out.append(('%s/%s' % (name, dt), (dt, sch, n, c, rels, ths, kw)))
    return out
