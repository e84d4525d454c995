"""The project's cases that run between guard bands (tests/guarded.py): the smallest parametrisation of every family that
still has tails, more than one part or split, and every element type of the family.  tests/test_guard_bands_emul.py runs
them on the host emulator, tests/test_gpu_guard_bands.py on the hardware; each case keeps its own assertions, the bands add
"and nothing within 4096 bytes outside any buffer changed".

CASES: (id, where, run) -- where: 'both', or 'emul' for the cases whose ranks are threads of one process (emulator only, as
in their own modules); run(x) with x.rt the guarded runtime, x.mp pytest's monkeypatch, x.where 'emulator' or 'GPU'."""
import numpy as np

import skfusion_amd._native as nat

import above_cases as AC
import api_cases
import complete_cases as CC
import dense_cases as DC
import filled_entries_cases as FE
import foldin_cases as FI
import known_cases as KN
import known_csr_cases as KC
import list_grid_cases as LG
import pinv_cases
import ranks_cases as RC
import sparse_dfmf_cases as SD
import sparse_foldin_cases as SF
import sparse_owned_cases as OC
import test_emul_kernels as K
import theta_csr_cases as TC
import theta_owned_cases as TO

F64, F32, MFMA, VALU = nat.SKF_F64, nat.SKF_F32, nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU
GEMM_SHAPE = (70, 130, 33)                  # row, column and K tails on every tile, three column blocks of the small tile
N_DENSE = {'a': 129, 'b': 67, 'c': 131}     # the smallest object counts off a multiple of 64 that hold rank 65
N_SMALL = {'a': 63, 'b': 65, 'c': 1}        # (the small-graph schedule holds ranks up to 64)
N_LISTS = {'a': 150, 'b': 130, 'c': 40}


def pinv_route(x, entry=None):
    """pinv_cases.run_pinv_strided on one matrix per route: the Cholesky inverse (verdict 1), the one-workgroup deflation
    (2), and an ambiguous spectrum that both decline (0: the eigen-solver; the matrix of
    test_pinv_ambiguous_spectrum_falls_back_to_the_exact_cut_off with lda = 28, ldk = 27)."""
    import scipy.linalg as spla
    if entry is not None:
        return K.test_pinv_with_leading_dimensions_above_the_order(x.rt, *entry)
    rs = np.random.RandomState(4)
    Qm, _ = np.linalg.qr(rs.randn(24, 24))
    A = (Qm * np.array([1.0] * 10 + [1e-8] * 2 + [0.0] * 12)) @ Qm.T
    A = 0.5 * (A + A.T)
    got, pad, verdict, _ = pinv_cases.run_pinv_strided(x.rt, F64, A, 28, 27)
    assert verdict == 0 and (pad == pinv_cases.POISON).all()
    assert K.relerr(got, spla.pinv(A)) < 1e-6


def dense(x, dtype, schedule, n, ranks, rels, thetas, **kw):
    DC.dense_case(dtype, schedule, n, ranks, rels, thetas, '%s guarded %s %s' % (x.where, schedule, dtype), x.mp, **kw)


def pipeline(x, dtype):
    dense(x, dtype, 'pipeline', N_DENSE, {'a': 65, 'b': 65, 'c': 65},
          [('a', 'b', 'neg', None), ('b', 'c', 'neg', None), ('c', 'a', 'pos', None)], [('a', 'csr')])


def staged(x, dtype, **kw):
    dense(x, dtype, 'staged', {'a': 129, 'b': 63}, {'a': 65, 'b': 8},
          [('a', 'b', 'neg', None), ('b', 'a', 'neg', None)], [('a', 'dense'), ('b', 'csr')], **kw)


def small(x, dtype, schedule):
    dense(x, dtype, schedule, N_SMALL, {'a': 64, 'b': 1, 'c': 5},
          [('a', 'b', 'neg', None), ('c', 'a', 'neg', None), ('b', 'c', 'pos', None)], [('a', 'csr')])


def dfmc(x, dtype):
    dense(x, dtype, 'staged', {'a': 129, 'b': 65}, {'a': 65, 'b': 8}, [('a', 'b', 'neg', 0.3)], [('a', 'csr')], **DC.DFMC)


def chain17(x, dtype):
    """pinv_cases.chain17_graph through a plan: 17 types, the second chunk of the pack / unpack launches; one iteration
    against the oracle under the bounds of test_fit_of_17_types."""
    from oracle import dfmf_oracle as orc
    from skfusion_amd._engine import small_graph_limits
    from skfusion_amd.fusion.decomposition import _dfmf
    R, types, rank, G0 = pinv_cases.chain17_graph()
    if len(types) <= small_graph_limits()['max_types']:
        x.mp.setenv('SKF_NO_SMALL_FUSED', '1')
    Go, So = orc.dfmf(R, {}, types, rank, max_iter=1, G0=G0)
    G, S = _dfmf.dfmf(R, {}, types, rank, max_iter=1, G0=G0, dtype=dtype)
    tol_g, tol_s = {'f64': (1e-7, 1e-7), 'f32': (1e-4, 1e-3), 'bf16': (2e-2, 2e-2)}[dtype]
    for t in types:
        assert K.relerr(G[t, t], Go[t, t]) < tol_g, t
    for k in So:
        assert K.relerr(S[k][0], So[k][0]) < tol_s, k


def above_retry(x, dtype):
    """DeviceCompleter.above with a capacity far below the count: SKF_E_WORKSPACE from the first call, the repeat with the
    count it reported -- the same arrays as the host."""
    from skfusion_amd._engine import DeviceCompleter
    G_row, S, G_col = CC.lattice_factors(67, 203, (5, 7))
    X = np.dot(np.dot(G_row, S), G_col.T)
    thr = AC.own_thresholds(X)
    ex = CC.exclusion_mask('edges', 67, 203)
    want = AC.host_above(X, thr, ex)
    assert want[0][-1] > 1
    got = DeviceCompleter(S, G_col, dtype=dtype).above(G_row, thr, exclude=CC.lists_of(ex), capacity=1, col_splits=3)
    AC.same(got, want, 'guarded above, capacity 1, %s' % dtype)


def entries(x, dtype):
    """skf_complete_entries on repeated pairs and the corners, raw and through the engine."""
    from skfusion_amd._engine import DeviceCompleter
    m, n_cols = 67, 203
    G_row, S, G_col = CC.lattice_factors(m, n_cols, (5, 7))
    H = np.dot(G_row, S)
    X = np.dot(H, G_col.T)
    rs = np.random.RandomState(3)
    rows = np.concatenate([[0, m - 1, 5, 5], rs.randint(0, m, 300)])
    cols = np.concatenate([[0, n_cols - 1, 2, 2], rs.randint(0, n_cols, 300)])
    assert np.array_equal(CC.Raw(dtype, H, G_col).entries(rows, cols).astype(np.float64), X[rows, cols])
    assert np.array_equal(DeviceCompleter(S, G_col, dtype=dtype).entries(G_row, rows, cols), X[rows, cols])


def fold(x, name):
    FI.fold_case(*FI.EMUL[name], what='%s guarded fold-in %s' % (x.where, name))


CASES = [
    # ---- stand-alone operators
    ('gemm_f64_mfma', 'both', lambda x: K.test_gemm_plain_all_layouts(x.rt, F64, MFMA, GEMM_SHAPE)),
    ('gemm_f64_valu', 'both', lambda x: K.test_gemm_plain_all_layouts(x.rt, F64, VALU, GEMM_SHAPE)),
    ('gemm_f32_mfma', 'both', lambda x: K.test_gemm_plain_all_layouts(x.rt, F32, MFMA, GEMM_SHAPE)),
    ('gemm_f32_valu', 'both', lambda x: K.test_gemm_plain_all_layouts(x.rt, F32, VALU, GEMM_SHAPE)),
    ('epilogues_f64_mfma', 'both', lambda x: K.test_gemm_epilogues_and_operand_ops(x.rt, F64, MFMA)),
    ('epilogues_f64_valu', 'both', lambda x: K.test_gemm_epilogues_and_operand_ops(x.rt, F64, VALU)),
    ('epilogues_f32_mfma', 'both', lambda x: K.test_gemm_epilogues_and_operand_ops(x.rt, F32, MFMA)),
    ('epilogues_f32_valu', 'both', lambda x: K.test_gemm_epilogues_and_operand_ops(x.rt, F32, VALU)),
    ('gemm_bf16', 'both', lambda x: K.test_gemm_bf16_contraction(x.rt, (130, 100, 70))),
    ('gemm_bf16_tn', 'both', lambda x: K.test_gemm_bf16_transposed_a(x.rt, (100, 130, 70))),
    ('gemm_bits', 'both', lambda x: K.test_gemm_bits_binary_relation_as_a_bitmap(x.rt, (70, 100, 130), 0)),
    ('gemm_bits_transposed', 'both', lambda x: K.test_gemm_bits_binary_relation_as_a_bitmap(x.rt, (70, 100, 130), 1)),
    ('to_bf16', 'both', lambda x: K.test_to_bf16_and_transpose(x.rt)),
    ('fill_uniform', 'both', lambda x: K.test_fill_uniform_matches_oracle_hash(x.rt)),
    ('fill_unknown', 'both', lambda x: api_cases.device_fill_strategies()),
    ('pinv_strided_cholesky', 'both', lambda x: pinv_route(x, K.STRIDED[0])),
    ('pinv_strided_deflation_f32', 'both', lambda x: pinv_route(x, K.STRIDED[3])),
    ('pinv_strided_eigen', 'both', lambda x: pinv_route(x)),
    ('pinv_order_257', 'both', lambda x: K.test_pinv_blocked_sweep_above_order_256(x.rt, 257)),
    # ---- one iteration of every schedule, all three element types
    ('pipeline_f64', 'both', lambda x: pipeline(x, 'f64')),
    ('pipeline_f32', 'both', lambda x: pipeline(x, 'f32')),
    ('pipeline_bf16', 'both', lambda x: pipeline(x, 'bf16')),
    ('staged_f64', 'both', lambda x: staged(x, 'f64')),
    ('staged_f32', 'both', lambda x: staged(x, 'f32', deficient='b')),
    ('staged_bf16', 'both', lambda x: staged(x, 'bf16')),
    ('small_graph_f64', 'both', lambda x: small(x, 'f64', 'small')),
    ('small_graph_f32', 'both', lambda x: small(x, 'f32', 'small')),
    ('no_small_fused_f64', 'both', lambda x: small(x, 'f64', 'chain')),
    ('no_small_fused_f32', 'both', lambda x: small(x, 'f32', 'chain')),
    ('no_small_fused_bf16', 'both', lambda x: small(x, 'bf16', 'chain')),
    ('dfmc_f32', 'both', lambda x: dfmc(x, 'f32')),
    ('chain17_f64', 'both', lambda x: chain17(x, 'f64')),
    ('chain17_f32', 'both', lambda x: chain17(x, 'f32')),
    ('chain17_bf16', 'both', lambda x: chain17(x, 'bf16')),
    # ---- entry lists
    ('known_lists_f64_parts4', 'both', lambda x: KN.list_case(203, 197, 64, 8, 'f64', 4, 'heavy', x.where + ' guarded', x.mp)),
    ('known_lists_f32_parts1', 'both', lambda x: KN.list_case(203, 197, 24, 8, 'f32', 1, 'edges', x.where + ' guarded', x.mp)),
    ('known_lists_bf16_parts4', 'both', lambda x: KN.list_case(203, 197, 128, 8, 'bf16', 4, 'edges', x.where + ' guarded', x.mp)),
    ('known_ones_parts1', 'both', lambda x: KN.ones_case(331, 333, 64, 128, 1, 'edges', x.where + ' guarded', x.mp)),
    ('known_ones_parts4', 'both', lambda x: KN.ones_case(331, 333, 256, 64, 4, 'full', x.where + ' guarded', x.mp)),
    ('known_csr_f64', 'both', lambda x: KC.csr_against_mask(N_LISTS, {'a': 20, 'b': 24, 'c': 5}, 0.06, 'f64', 4, x.mp)),
    ('known_csr_f32', 'both', lambda x: KC.csr_against_mask(N_LISTS, {'a': 64, 'b': 24, 'c': 5}, 0.06, 'f32', 1, x.mp)),
    ('known_csr_bf16', 'both', lambda x: KC.csr_against_mask(N_LISTS, {'a': 64, 'b': 24, 'c': 5}, 0.06, 'bf16', 4, x.mp)),
    ('stored_pass_f64', 'both', lambda x: SD.pass_case(203, 197, 16, 20, 'f64', 4, 'edges', x.where + ' guarded', x.mp, seed=4)),
    ('stored_pass_f32', 'both', lambda x: SD.pass_case(203, 197, 32, 24, 'f32', 1, 'heavy', x.where + ' guarded', x.mp, seed=1)),
    ('stored_pass_bf16', 'both', lambda x: SD.pass_case(203, 197, 64, 128, 'bf16', 4, 'full', x.where + ' guarded', x.mp, seed=4)),
    ('stored_lists_f64', 'both', lambda x: SD.lists_case(150, 130, 64, 24, 'f64', 1, 0.06, x.mp, seed=1)),
    ('stored_lists_f32', 'both', lambda x: SD.lists_case(259, 67, 20, 64, 'f32', 4, 0.05, x.mp, seed=3, edits=('empty', 'full_row'))),
    ('stored_lists_bf16', 'both', lambda x: SD.lists_case(150, 130, 64, 24, 'bf16', 4, 0.06, x.mp, seed=4)),
    ('filled_pass_f64', 'both', lambda x: FE.pass_case(203, 197, 5, 15, 'f64', 4, 'edges', x.where + ' guarded', x.mp, seed=4, lengths=(1, 4, 5, 16, 17, 64, 65))),
    ('filled_pass_f32', 'both', lambda x: FE.pass_case(203, 197, 32, 16, 'f32', 1, 'full', x.where + ' guarded', x.mp, seed=1, lengths=(1, 4, 5, 16, 17, 64, 65))),
    ('filled_pass_bf16', 'both', lambda x: FE.pass_case(203, 197, 64, 128, 'bf16', 4, 'heavy', x.where + ' guarded', x.mp, seed=4, lengths=(1, 4, 5, 16, 17, 64, 65))),
    ('grid_known_f64', 'both', lambda x: LG.known_case((5, 33), 8, 'f64', 8, x.where + ' guarded grid known', x.mp)),
    ('grid_known_f32', 'both', lambda x: LG.known_case((5, 33), 8, 'f32', 8, x.where + ' guarded grid known', x.mp)),
    ('grid_known_bf16', 'both', lambda x: LG.known_case((5, 33), 128, 'bf16', 8, x.where + ' guarded grid known', x.mp)),
    ('grid_stored_f64', 'both', lambda x: LG.stored_case((5, 33), 8, 'f64', 8, x.where + ' guarded grid stored', x.mp)),
    ('grid_stored_f32', 'both', lambda x: LG.stored_case((5, 33), 8, 'f32', 8, x.where + ' guarded grid stored', x.mp)),
    ('grid_stored_bf16', 'both', lambda x: LG.stored_case((5, 33), 128, 'bf16', 8, x.where + ' guarded grid stored', x.mp)),
    ('grid_filled_f64', 'both', lambda x: LG.filled_case((5, 33), 8, 'f64', 8, x.where + ' guarded grid filled', x.mp)),
    ('grid_filled_f32', 'both', lambda x: LG.filled_case((5, 33), 8, 'f32', 8, x.where + ' guarded grid filled', x.mp)),
    ('grid_filled_bf16', 'both', lambda x: LG.filled_case((5, 33), 128, 'bf16', 8, x.where + ' guarded grid filled', x.mp)),
    ('grid_ones', 'both', lambda x: LG.ones_case((64, 128), 8, 'edges', x.where + ' guarded grid ones', x.mp)),
    ('grid_fold_f64', 'both', lambda x: LG.fold_case((5, 33), 8, 'f64', x.where + ' guarded grid fold-in')),
    ('grid_fold_f32', 'both', lambda x: LG.fold_case((5, 33), 8, 'f32', x.where + ' guarded grid fold-in')),
    ('grid_fold_bf16', 'both', lambda x: LG.fold_case((5, 33), 128, 'bf16', x.where + ' guarded grid fold-in')),
    ('fold_lists_f64', 'both', lambda x: SF.fold_lists_case(37, 41, 65, 'edges', 'f64')),
    ('fold_lists_f32', 'both', lambda x: SF.fold_lists_case(37, 41, 5, 'heavy', 'f32')),
    ('fold_whole_f64', 'both', lambda x: SF.whole_case('f64', {'t': 8, 'a': 20, 'b': 8}, True, x.where + ' guarded', n={'t': 37, 'a': 41, 'b': 30})),
    ('fold_whole_f32', 'both', lambda x: SF.whole_case('f32', {'t': 70, 'a': 8, 'b': 20}, False, x.where + ' guarded', n={'t': 37, 'a': 41, 'b': 30})),
    ('fold_whole_bf16', 'both', lambda x: SF.whole_case('bf16', {'t': 64, 'a': 128, 'b': 256}, True, x.where + ' guarded')),
    ('foldin_fused_f64', 'both', lambda x: fold(x, 'fused_f64_big')),
    ('foldin_fused_f32', 'both', lambda x: fold(x, 'fused_f32_one')),
    ('foldin_fused_bf16', 'both', lambda x: fold(x, 'fused_bf16')),
    ('foldin_generic_f32_csr', 'both', lambda x: fold(x, 'generic_f32_csr')),
    ('foldin_generic_bf16_dense', 'both', lambda x: fold(x, 'generic_bf16_dense')),
    ('foldin_batch17', 'both', lambda x: FI.batch_case(*FI.EMUL_BATCH['batch17_f64'], what=x.where + ' guarded fold-in batch')),
    # ---- constraints
    ('theta_entries_f64_small_graph', 'both', lambda x: TC.entries_against_dense('dfmf', 'f64', 20, x.mp, expect_small=True)),
    ('theta_entries_f32_general', 'both', lambda x: TC.entries_against_dense('dfmf', 'f32', 20, x.mp, general=True, expect_small=False)),
    ('theta_entries_bf16', 'both', lambda x: TC.entries_against_dense('dfmf', 'bf16', 70, x.mp, expect_small=False)),
    ('theta_hub_f64', 'both', lambda x: TC.hub_case('f64', 65, x.mp, n=150)),
    ('theta_hub_f32', 'both', lambda x: TC.hub_case('f32', 5, x.mp, n=150)),
    ('theta_hub_bf16', 'both', lambda x: TC.hub_case('bf16', 65, x.mp, n=150)),
    ('theta_half_full_f64', 'both', lambda x: TC.half_full_case('f64', x.where)),
    ('theta_half_full_f32', 'both', lambda x: TC.half_full_case('f32', x.where)),
    ('theta_half_full_bf16', 'both', lambda x: TC.half_full_case('bf16', x.where)),
    ('theta_owned_hub_bits_f64', 'emul', lambda x: TO.hub_bits_case('f64', 65, 2, 64, x.mp)),
    ('theta_owned_hub_bits_f32', 'emul', lambda x: TO.hub_bits_case('f32', 5, 3, 64, x.mp)),
    ('theta_owned_hub_bits_bf16', 'emul', lambda x: TO.hub_bits_case('bf16', 65, 2, 64, x.mp)),
    # ---- owned rows
    ('owned_lists_zero', 'emul', lambda x: OC.lists_case('f64', 3, 4, 'zero', x.mp, seed=7)),
    ('owned_lists_unknown', 'emul', lambda x: OC.lists_case('bf16', 2, 4, 'unknown', x.mp, seed=6)),
    # ---- completion
    # (203 columns are four tiles: asked for three parts the launch forms two and a third that is empty, so the last slot of
    # the partial lists is written with two parts -- and k = 64 makes a slot 256 bytes, the granule of the sizes)
    ('topk_f64', 'both', lambda x: CC.exact_case('f64', 67, 203, (5, 7), ks=(64,), splits=(1, 2, 3))),
    ('topk_f32', 'both', lambda x: CC.exact_case('f32', 67, 203, (5, 7), ks=(64,), splits=(1, 2, 3))),
    ('ranks_f64', 'both', lambda x: RC.exact_case('f64', 67, 203, (5, 7))),
    ('ranks_f32', 'both', lambda x: RC.exact_case('f32', 67, 203, (5, 7))),
    ('above_f64', 'both', lambda x: AC.exact_case('f64', 67, 203, (5, 7))),
    ('above_f32', 'both', lambda x: AC.exact_case('f32', 67, 203, (5, 7))),
    ('above_scan_f64', 'both', lambda x: AC.scan_case('f64', 600)),
    ('above_scan_f32', 'both', lambda x: AC.scan_case('f32', 600)),
    ('above_seam_f64', 'both', lambda x: AC.seam_case('f64')),
    ('above_seam_f32', 'both', lambda x: AC.seam_case('f32')),
    ('above_retry_f64', 'both', lambda x: above_retry(x, 'f64')),
    ('above_retry_f32', 'both', lambda x: above_retry(x, 'f32')),
    ('complete_entries_f64', 'both', lambda x: entries(x, 'f64')),
    ('complete_entries_f32', 'both', lambda x: entries(x, 'f32')),
]


class Context(object):
    def __init__(self, rt, mp, where):
        self.rt, self.mp, self.where = rt, mp, where


def run_guarded(case_id, monkeypatch, where, rt=None):
    """One case of CASES between guard bands; returns (buffers, bands) checked."""
    from guarded import guarded
    run = {c[0]: c[2] for c in CASES}[case_id]
    with guarded(rt, label=case_id) as g:
        run(Context(g.rt, monkeypatch, where))
    assert g.buffers > 0 and g.bands == 2 * g.buffers
    return g.buffers, g.bands
