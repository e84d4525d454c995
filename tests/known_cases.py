"""DFMC on the known entries only (skf_relation_desc.known_bound, csrc/skf_known.h) against the dense path that keeps the
completed relation -- the SAME cases on the host emulator (small) and on the GPU (large ranks, all list-pass kernels).
The dense path itself is pinned to the reference's goldens elsewhere; the two formulations differ by associativity only
(reference _dfmc.py:287-292, 311-325, 341-352), so in f64 they must agree to rounding.
Second half: every list kernel variant held to a host model of one iteration (list_case, ones_case; error model below)."""
import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd._engine import DevicePlan
from helpers import relerr, within


def masked_graph(n, ranks, known_share, seed=0):
    """a x b ratings-like relation with `known_share` of its entries known, an unmasked b x c relation, a second masked
    a x c relation (denser), and a constraint on b."""
    rs = np.random.RandomState(seed)
    types = ['a', 'b', 'c']
    Ga = rs.rand(n['a'], 4)
    Gb = rs.rand(n['b'], 4)
    R_ab = (Ga @ rs.rand(4, 4) @ Gb.T) / 4.0 + 0.05 * rs.rand(n['a'], n['b'])
    M_ab = rs.rand(n['a'], n['b']) >= known_share                 # True = unknown
    R_bc = (rs.rand(n['b'], n['c']) < 0.2).astype(np.float64)
    R_ac = rs.rand(n['a'], n['c'])
    M_ac = rs.rand(n['a'], n['c']) >= min(4 * known_share, 0.2)
    theta = -0.01 * (rs.rand(n['b'], n['b']) < 2.0 / n['b'])
    theta = theta + theta.T
    np.fill_diagonal(theta, 0.02)
    rels = [('a', 'b', R_ab, M_ab), ('b', 'c', R_bc, None), ('a', 'c', R_ac, M_ac)]
    thetas = [('b', theta)]
    G0 = {t: rs.rand(n[t], ranks[t]) + 0.1 for t in types}
    return types, rels, thetas, G0


def run(types, n, ranks, rels, thetas, G0, dtype, iters, sparse, with_errors=False):
    plan = DevicePlan(types, n, ranks, rels, thetas, nat.SKF_DFMC, dtype=dtype, sparse_known=None if sparse else False)
    try:
        for t in types:
            plan.set_factor(t, G0[t])
        errs = []
        if with_errors:
            for _ in range(iters):
                plan.iterate(1)
                errs.append([plan.relation_sqerr(k) for k in range(len(rels))])
        else:
            plan.iterate(iters)
        G = {t: plan.get_factor(t) for t in types}
        S = [plan.get_backbone(k) for k in range(len(rels))]
        extra = {}
        if sparse:
            extra['A'] = plan.get_contraction(0, 2)
            extra['Q'] = plan.get_contraction(0, 1)
        else:
            extra['P'] = plan.get_contraction(0, 0)
            extra['Q'] = plan.get_contraction(0, 1)
            extra['S'] = S[0]
        return G, S, np.array(errs), extra
    finally:
        plan.close()


def sparse_against_dense(n, ranks, known_share, iters, dtype, tol, what, monkeypatch, parts=1, seed=0):
    """Same graph, same start: lists of known entries vs completed dense copy.  tol = (G, S, squared errors, P S^T, Q)."""
    tol_g, tol_s, tol_e, tol_a, tol_q = tol
    monkeypatch.setenv('SKF_DFMC_SPARSE', '1')              # whenever a bound is given (up to a quarter known)
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    types, rels, thetas, G0 = masked_graph(n, ranks, known_share, seed)
    Gs, Ss, Es, xs = run(types, n, ranks, rels, thetas, G0, dtype, iters, True, with_errors=True)
    Gd, Sd, Ed, xd = run(types, n, ranks, rels, thetas, G0, dtype, iters, False, with_errors=True)
    for t in types:
        within(relerr(Gs[t], Gd[t]), tol_g, '%s: known-entries DFMC vs dense, G_%s after %d iterations' % (what, t, iters))
    for k in range(len(rels)):
        within(relerr(Ss[k], Sd[k]), tol_s, '%s: known-entries DFMC vs dense, S_%d' % (what, k))
    within(np.max(np.abs(Es - Ed) / Ed), tol_e, '%s: known-entries DFMC vs dense, squared errors of every iteration' % what)
    # the row-side product the lists form instead of P:  A = P S^T  (dense path: P and S of the same iteration)
    within(relerr(xs['A'], xd['P'].astype(np.float64) @ xd['S'].T), tol_a, '%s: row-side product P S^T' % what)
    within(relerr(xs['Q'], xd['Q']), tol_q, '%s: column contraction Q' % what)
    return Gs, Ss


# ---- the list kernels held to host arithmetic (one iteration, every kernel variant, masks built for the kernels' edges) ----
#
# Error model (every bound of list_case / ones_case below).  The host repeats the engine's operand roundings and nothing
# else: bf16 -- bf16 rows of G_i and of T = G_j S^T, r as the bf16 value the relation is stored in, f32 accumulation;
# f32 -- f32 operands and accumulation; f64 -- no rounding.  The c x c parts (S Gram_j S^T, S^T Gram_i) come from the
# f32 / f64 masters in f64.  What remains between device and host is then
#   (a) the accumulation of the list pass: x = <Fo, Fi> over w = c_i terms, e = r - x, then e * Fi over the L entries of
#       the list and the fixed-order sums over lane groups and parts -- at most n = w + L + parts + 2 roundings of unit u
#       (2^-24 for f32 accumulation, 2^-53 for f64) on any element, so with M = |E| |T| + (K o (|G_i| |T|^T)) |T| (row
#       side; column side |E|^T |G_i| + (K o (|G_i| |T|^T))^T |G_i|) the classical bound  |delta| <= n u M  element-wise;
#   (b) T itself: the device forms T = G_j S^T with an inner dimension c_j (error <= (c_j + 2) u |G_j| |S|^T) and rounds
#       it to the gathered type; a value that lies that close to a rounding boundary of bf16 (a midpoint) may round either
#       way on the device.  Allowed for EXPLICITLY: dT = the largest distance between the host's rounded T and the
#       rounded ends of [T - err, T + err] (0 wherever both ends round to the same bf16 value), and dT enters the bound at
#       first order: |E| dT + (K o (|G_i| dT^T)) (|T| + dT) on the row side, (K o (|G_i| dT^T))^T |G_i| on the column side;
#   (c) the dense part the engine adds to the sparse term (A = G_i Bf + E T, Q = G_j U2 + E^T G_i): its c x c operand
#       formed in f64 from Gram matrices summed over the n objects of a type, (n + c_i + c_j + 2) 2^-53 |S| |G_j|^T |G_j| |S|^T
#       for Bf (|S|^T |G_i|^T |G_i| for U2) -- the term that matters in the f64 engine --, then the product with G in the
#       master type, (c + 2) u |G| |Bf|, and the final rounding u |A|.
# Each bound is K_SAFE = 2 times the sum of these first-order terms (the factor covers the second-order terms the
# first-order sums leave out), and it is applied element by element to the SPARSE term on its own: A - G_i Bf against E T,
# Q - G_j U2 against E^T G_i -- a kernel that drops one entry of a list moves an element by |e| |T_q|, about M / L, far
# above n u M for every list length used here.  The squared error of skf_relation_sqerr (one SRP_ERR pass over the column
# lists with the residuals the last iteration stored) gets the same treatment: its list sum against the host's, with the
# f32 rounding of every (r - x)^2 term and the propagation of dx, de, plus the f64 rounding of the trace terms the engine
# evaluates from c x c Gram matrices.
K_SAFE = 2.0
LIST_LENGTHS = (1, 4, 5, 12, 13, 16, 17, 63, 64, 65, 128, 129)
U_ACC = {'f64': 2.0 ** -53, 'f32': 2.0 ** -24, 'bf16': 2.0 ** -24}


def bf16_round(x):
    return nat.from_bf16_bits(nat.to_bf16_bits(np.asarray(x, dtype=np.float32))).astype(np.float64)


def store_round(x, dtype):
    """f64 -> the value the engine gathers: bf16 (through f32, as the device converts its f32 T), f32, or f64 itself."""
    if dtype == 'bf16':
        return bf16_round(x)
    if dtype == 'f32':
        return np.asarray(x, dtype=np.float32).astype(np.float64)
    return np.asarray(x, dtype=np.float64)


def gathered_T(Gj, S, dtype):
    """T = G_j S^T as the engine gathers it, and dT: how far the device's value may lie from the host's (model (b))."""
    T = Gj @ S.T
    err = (Gj.shape[1] + 2) * U_ACC[dtype] * (np.abs(Gj) @ np.abs(S).T)
    Tr = store_round(T, dtype)
    dT = np.maximum(np.abs(store_round(T + err, dtype) - Tr), np.abs(Tr - store_round(T - err, dtype)))
    return Tr, dT


def edge_mask(n_a, n_b, pattern, seed, lengths=LIST_LENGTHS, bg=0.03):
    """KNOWN pattern (True = known) built for the edges of the list kernels.
    edges:  an empty row and an empty column; rows 0.. / columns 0.. with exactly the known entries of `lengths` (batches
            of 64, the 4 / 8 / 12 / 16 chunk cut-offs of srp_bf16_v6_kernel), each including the LAST column / row (next
            to the zero row the v6 kernel reads past list ends); a row and a column known only in the last of 8 parts,
            a row and a column known on both sides of every part boundary of 2 / 4 / 8 parts; background share `bg`.
    full:   one row and one column (the last) known across their whole length -- several batches, every part boundary.
    heavy:  a heavy-tailed degree distribution like real ratings (Zipf-like row degrees and column popularities)."""
    rs = np.random.RandomState(seed)
    K = np.zeros((n_a, n_b), dtype=bool)
    if pattern == 'heavy':
        deg = np.minimum(n_b, np.floor(bg * n_b * 6.0 / (1.0 + np.arange(n_a)) ** 0.7) + 1).astype(int)
        rs.shuffle(deg)
        pop = 1.0 / (1.0 + np.arange(n_b)) ** 0.8
        rs.shuffle(pop)
        pop /= pop.sum()
        for o in range(n_a):
            K[o, rs.choice(n_b, deg[o], replace=False, p=pop)] = True
        return K
    if pattern == 'full':
        K = rs.rand(n_a, n_b) < bg
        K[n_a // 2, :] = True
        K[:, n_b - 1] = True
        return K
    assert pattern == 'edges'
    lens = [L for L in lengths if L <= min(n_a, n_b) - 24]
    nl = len(lens)
    er, ec = nl, nl                                   # the empty row / column
    lr, lc = nl + 1, nl + 1                           # known only in the last of 8 parts
    br, bc = nl + 2, nl + 2                           # both sides of every part boundary
    first = nl + 3
    K[first:, first:] = rs.rand(n_a - first, n_b - first) < bg
    K[first:, n_b - 1] |= rs.rand(n_a - first) < 0.5
    for k, L in enumerate(lens):                      # rows / columns of exact length, the last column / row included
        K[k, rs.choice(np.arange(first, n_b - 1), L - 1, replace=False)] = True
        K[k, n_b - 1] = True
        K[rs.choice(np.arange(first, n_a - 1), L - 1, replace=False), k] = True
        K[n_a - 1, k] = True
    pw8 = ((n_b + 7) // 8 + 63) // 64 * 64
    ph8 = ((n_a + 7) // 8 + 63) // 64 * 64
    K[lr, max(first, 7 * pw8):] = True
    K[max(first, 7 * ph8):, lc] = True
    for parts in (2, 4, 8):
        pw = ((n_b + parts - 1) // parts + 63) // 64 * 64
        ph = ((n_a + parts - 1) // parts + 63) // 64 * 64
        for q in range(1, parts):
            K[br, [c for c in (q * pw - 1, q * pw) if first <= c < n_b]] = True
            K[[r for r in (q * ph - 1, q * ph) if first <= r < n_a], bc] = True
    K[er, :] = False
    K[:, ec] = False
    return K


def list_case(n_a, n_b, c_a, c_b, dtype, parts, pattern, what, monkeypatch, seed=0, lengths=LIST_LENGTHS):
    """One masked a x b relation kept as lists of its known entries (`pattern`, edge_mask), DFMC on the engine `dtype` with
    the lists in `parts` parts: after one iteration from G0, the factors (G_i, G_j) are read, one more iteration runs and
    the row-side product A = P S^T, the column contraction Q and the relation's squared error are held to the host model
    of that iteration (see the error model above).  Returns the measured worst |delta| / bound of each check."""
    monkeypatch.setenv('SKF_DFMC_SPARSE', '1')
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    rs = np.random.RandomState(seed)
    K = edge_mask(n_a, n_b, pattern, seed, lengths)
    assert 0 < K.sum() <= 0.25 * K.size
    R = rs.rand(n_a, n_b) * 2.0                     # not low rank: residuals of order one on every known entry
    G0 = {'a': rs.rand(n_a, c_a) + 0.1, 'b': rs.rand(n_b, c_b) + 0.1}
    types, n, ranks = ['a', 'b'], {'a': n_a, 'b': n_b}, {'a': c_a, 'b': c_b}
    plan = DevicePlan(types, n, ranks, [('a', 'b', R, ~K)], [], nat.SKF_DFMC, dtype=dtype)
    try:
        for t in types:
            plan.set_factor(t, G0[t])
        plan.iterate(1)
        Gi, Gj = plan.get_factor('a').astype(np.float64), plan.get_factor('b').astype(np.float64)
        plan.iterate(1)
        S = plan.get_backbone(0).astype(np.float64)
        A = plan.get_contraction(0, 2).astype(np.float64)
        Q = plan.get_contraction(0, 1).astype(np.float64)
        with pytest.raises(nat.SkfNativeError):
            plan.get_contraction(0, 0)               # the list path is the one that ran: it never forms P
        sq = plan.relation_sqerr(0)
        Gi2, Gj2 = plan.get_factor('a').astype(np.float64), plan.get_factor('b').astype(np.float64)
    finally:
        plan.close()
    u = U_ACC[dtype]
    Kf = K.astype(np.float64)
    r = store_round(R, dtype)                                           # (the relation as the engine stores it)
    Gib = store_round(Gi, dtype)
    Tb, dT = gathered_T(Gj, S, dtype)
    X = Gib @ Tb.T
    E = np.where(K, r - X, 0.0)
    absG, absT = np.abs(Gib), np.abs(Tb)
    absX = Kf * (absG @ absT.T)                                         # K o (|G_i| |T|^T)
    dX = Kf * (absG @ dT.T)                                             # what dT does to the dot products
    L_row, L_col = K.sum(1).astype(np.float64)[:, None], K.sum(0).astype(np.float64)[:, None]
    ratios = {}

    # row side: A - G_i Bf against E T
    Bf = S @ (Gj.T @ Gj) @ S.T
    dense = Gi @ Bf
    M = np.abs(E) @ absT + absX @ absT
    bound = (c_a + L_row + parts + 2) * u * M + np.abs(E) @ dT + dX @ (absT + dT)
    dBf = (n_b + c_a + c_b + 2) * 2.0 ** -53 * (np.abs(S) @ (np.abs(Gj).T @ np.abs(Gj)) @ np.abs(S).T)
    bound += (c_a + 2) * u * (np.abs(Gi) @ np.abs(Bf)) + np.abs(Gi) @ dBf + u * np.abs(A)
    dev = np.abs((A - dense) - E @ Tb)
    ratios['row-side sparse term E T'] = np.max(dev / (K_SAFE * bound))
    # column side: Q - G_j U2 against E^T G_i
    U2 = S.T @ (Gi.T @ Gi)
    dense = Gj @ U2
    M = np.abs(E).T @ absG + absX.T @ absG
    bound = (c_a + L_col + parts + 2) * u * M + dX.T @ absG
    dU2 = (n_a + c_a + c_b + 2) * 2.0 ** -53 * (np.abs(S).T @ (np.abs(Gi).T @ np.abs(Gi)))
    bound += (c_b + 2) * u * (np.abs(Gj) @ np.abs(U2)) + np.abs(Gj) @ dU2 + u * np.abs(Q)
    dev = np.abs((Q - dense) - E.T @ Gib)
    ratios['column-side sparse term E^T G_i'] = np.max(dev / (K_SAFE * bound))
    # squared error: |X_o - X_n|^2 (trace terms, f64) + sum over the known entries of (r - x_n)^2 - (r - e - x_n)^2
    Xo, Xn = Gi @ S @ Gj.T, Gi2 @ S @ Gj2.T
    trace = np.sum((Xo - Xn) ** 2)
    aXo, aXn = np.abs(Gi) @ np.abs(S) @ np.abs(Gj).T, np.abs(Gi2) @ np.abs(S) @ np.abs(Gj2).T
    Gib2 = store_round(Gi2, dtype)
    Tb2, dT2 = gathered_T(Gj2, S, dtype)
    xn = Gib2 @ Tb2.T
    dxn = (c_a + 2) * u * (np.abs(Gib2) @ np.abs(Tb2).T) + np.abs(Gib2) @ dT2.T
    de = (c_a + 2) * u * (absG @ absT.T) + np.abs(Gib) @ dT.T + u * np.abs(E)
    a1, a2 = r - xn, r - E - xn
    sparse = np.sum(Kf * (a1 ** 2 - a2 ** 2))
    bound = np.sum(Kf * (2 * np.abs(a1) * dxn + 2 * np.abs(a2) * (dxn + de) + 4 * u * (a1 ** 2 + a2 ** 2)))
    bound += (n_a + n_b + 2 * (c_a + c_b)) * 2.0 ** -53 * np.sum((aXo + aXn) ** 2)
    ratios['squared error, list sum (SRP_ERR pass)'] = abs(sq - trace - sparse) / (K_SAFE * bound)
    for k, v in ratios.items():
        within(v, 1.0, '%s: %s, |delta| / model bound' % (what, k))
    return ratios


def ones_case(n_a, n_b, c_a, c_b, parts, pattern, what, monkeypatch, seed=0, lengths=LIST_LENGTHS, bg=0.001):
    """A sparse 0 / 1 relation (at most one entry in 80 set) kept as lists over the bf16 factor rows
    (srp_bf16_v6_kernel<.., SRP_ONES, ..>, rank of the gathered factor 64 / 128 / 256; segment pointers of the parts from
    parted_ptr_kernel): P = R G_j and Q = R^T G_i of one iteration against f64 sums of the bf16 rows.  Model: sums of
    exact bf16 values in f32 -- |delta| <= (L + parts + 2) u (R |G|) element-wise (times K_SAFE)."""
    monkeypatch.setenv('SKF_KNOWN_PARTS', str(parts))
    rs = np.random.RandomState(seed)
    K = edge_mask(n_a, n_b, pattern, seed, lengths, bg)
    assert 0 < K.sum() <= K.size // 80
    R = K.astype(np.float64)
    G0 = {'a': rs.rand(n_a, c_a) + 0.1, 'b': rs.rand(n_b, c_b) + 0.1}
    types, n, ranks = ['a', 'b'], {'a': n_a, 'b': n_b}, {'a': c_a, 'b': c_b}
    plan = DevicePlan(types, n, ranks, [('a', 'b', R, None)], [], nat.SKF_DFMF, dtype='bf16')
    try:
        for t in types:
            plan.set_factor(t, G0[t])
        plan.iterate(1)
        Gi, Gj = plan.get_factor('a').astype(np.float64), plan.get_factor('b').astype(np.float64)
        plan.set_profiling(True)
        plan.iterate(1)
        nnz, read = int(K.sum()), plan.get_profile()[3]
        # the lists ran: 4 bytes per one and contraction (skf_plan_get_profile), not the bitmap's n_a * n_b / 8
        assert read == 8.0 * nnz, (read, nnz)
        P = plan.get_contraction(0, 0).astype(np.float64)
        Q = plan.get_contraction(0, 1).astype(np.float64)
    finally:
        plan.close()
    u = U_ACC['bf16']
    Gib, Gjb = bf16_round(Gi), bf16_round(Gj)
    out = {}
    for name, got, want, mag, L in (('P = R G_j', P, R @ Gjb, R @ np.abs(Gjb), R.sum(1)[:, None]),
                                    ('Q = R^T G_i', Q, R.T @ Gib, R.T @ np.abs(Gib), R.sum(0)[:, None])):
        bound = (L + parts + 2) * u * mag
        dev = np.abs(got - want)
        # (an empty list must give exactly 0: a bound of 0 there, and any deviation from it counts as infinitely far)
        out[name] = np.max(np.where(dev == 0, 0.0, dev / np.maximum(K_SAFE * bound, 1e-300)))
        within(out[name], 1.0, '%s: 0/1 relation as lists, %s, |delta| / model bound' % (what, name))
    return out
