"""Parity tests proper: the HIP engine on a real MI355X, called through the C ABI
(libskfusion_hip.so), against the golden vectors of the reference and the CPU oracle.
Run with `pytest -m gpu`.  Tolerances: the bounds marked `within(...)` are at most 10x the LARGEST deviation any check of
that call site measured (round 5: re-derived from profiles/r04_test_deviations.txt; rounding-level f64 checks keep a floor of
~20 ulp, said where they do), measured on the hardware (quoted next to them; every session writes measured vs bound to
gpurun_out/test_deviations.txt -> profiles/).  f64 vs the goldens of the reference: after 100
iterations on the README graph 2.5e-12 (`random`), 1.5e-10 (`random_vcol`), 1e-9 (`random_c`) -- measured
5.5e-13 / 3.6e-11 / 2.2e-10: SURVEY.md 8d's 1e-10 holds for `random` and at iterations 1-10, the
ill-conditioned column-mean initialisers drift to 2e-10 by iteration 100 --, 5e-9 / 2.5e-9 on dicty
(cond 4e5), 1.5e-11 on the scaled config 5; f32 <= 1e-4 on G / 1e-3 on S
after 30 iterations and <= 1e-5 relative on the per-relation reconstruction error."""
import numpy as np
import pytest

import skfusion_amd._native as nat
from skfusion_amd.fusion.decomposition import _dfmf, _dfmc
from skfusion_amd._engine import DevicePlan, DeviceMatrix, fill_uniform
from oracle import dfmf_oracle as orc
from helpers import (golden, readme_graph, probe_graph, rank_deficient_graph, dicty_graph,
                     c3_scaled_graph, g0_from, Snapshots, compare_snapshots, relerr, within, TYPES)
import test_emul_kernels as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rt():
    return nat.get_runtime()           # raises if libskfusion_hip.so or the GPU is missing


def test_native_library_is_the_one_loaded(rt):
    assert rt.name == 'hip'
    assert b'gfx950' in rt.lib.skf_version()


# ---- kernels (same checks as the emulator suite, on the hardware) -----------------------------
@pytest.mark.parametrize('dtype', [nat.SKF_F64, nat.SKF_F32])
@pytest.mark.parametrize('engine', [nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU])
@pytest.mark.parametrize('shape', K.SHAPES + [(1000, 256, 3000), (300, 128, 5000)])
def test_gemm_all_layouts(rt, dtype, engine, shape):
    K.test_gemm_plain_all_layouts(rt, dtype, engine, shape)


@pytest.mark.parametrize('dtype', [nat.SKF_F64, nat.SKF_F32])
@pytest.mark.parametrize('engine', [nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU])
def test_gemm_epilogues(rt, dtype, engine):
    K.test_gemm_epilogues_and_operand_ops(rt, dtype, engine)


@pytest.mark.parametrize('dtype', [nat.SKF_F64, nat.SKF_F32])
def test_gemm_split_k(rt, dtype):
    K.test_gemm_split_k_and_nan_to_num(rt, dtype)


@pytest.mark.parametrize('dtype', [nat.SKF_F64, nat.SKF_F32])
@pytest.mark.parametrize('engine', [nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU])
def test_gemm_strides_and_alignment(rt, dtype, engine):
    K.test_gemm_strides_and_alignment(rt, dtype, engine)


@pytest.mark.parametrize('dtype', [nat.SKF_F64, nat.SKF_F32])
def test_gemm_many_slices(rt, dtype):
    K.test_gemm_many_slices(rt, dtype)


@pytest.mark.parametrize('op', ['plain', 'plain256', 'tn', 'bits0', 'bits1'])
def test_gemm_bf16_reduce_layouts(rt, op):
    K.test_gemm_bf16_reduce_layouts(rt, op)


def test_workspaces_are_exact(rt):
    K.test_workspaces_are_exact(rt)


def test_mfma_and_valu_engines_agree_bitwise_in_f32(rt):
    """v_mfma_f32_32x32x2_f32 is an exact k-ordered fma chain: identical to the VALU kernel when
    the K tiling is the same chain order (single K slice)."""
    rs = np.random.RandomState(3)
    A, B = rs.randn(200, 300), rs.randn(300, 150)
    a, _ = K.run_gemm(rt, nat.SKF_F32, nat.SKF_ENGINE_MFMA, A, B, splits=1)
    b, _ = K.run_gemm(rt, nat.SKF_F32, nat.SKF_ENGINE_VALU, A, B, splits=1)
    assert relerr(a, b) < 1e-6


@pytest.mark.parametrize('n', [1, 2, 5, 10, 31, 50, 128, 256])
def test_pinv_full_rank(rt, n):
    K.test_pinv_full_rank_matches_scipy(rt, n)


@pytest.mark.parametrize('n', [65, 96, 130, 200, 256])
def test_pinv_blocked_sweep(rt, n):
    """Orders 65 .. 256 on the hardware: one launch per block step (sweep_step_kernel, the default) against scipy and the
    blocked Cholesky inverse, and bit for bit against one workgroup per matrix (sweep_inverse_kernel)."""
    K.test_pinv_blocked_sweep_orders_65_to_256(rt, n)
    K.test_pinv_sweep_one_launch_per_block_step_keeps_the_bits(rt, n)


@pytest.mark.parametrize('n', [257, 300, 420, 512, 777, 1023])
def test_pinv_blocked_sweep_above_order_256(rt, n):
    """Orders 257 .. 1023 on the hardware (sweep_step_kernel<true>: column operands from memory)."""
    K.test_pinv_blocked_sweep_above_order_256(rt, n)


def test_pinv_rank_deficient(rt):
    K.test_pinv_rank_deficient_truncates_like_scipy(rt)
    K.test_pinv_zero_and_diagonal(rt)


@pytest.mark.parametrize('n,rank', [(257, 1), (300, 170), (420, 97), (512, 256), (777, 300), (1023, 512), (1023, 700)])
def test_pinv_deflation_over_several_workgroups(rt, n, rank, monkeypatch):
    """Round 6: rank-deficient Gram matrices above order 256 on the hardware -- block-pivoted Cholesky steps over row slabs,
    gated finishing products, the fast path's sweep on L^T L (route asserted by the operator's verdict word); and the ambiguous
    spectrum that both deflations must leave to the eigen-solver."""
    K.test_pinv_deflation_over_several_workgroups_above_order_256(rt, n, rank, monkeypatch)


def test_pinv_ambiguous_spectrum_above_order_256(rt):
    K.test_pinv_ambiguous_spectrum_above_order_256_is_left_to_the_exact_cut_off(rt)


@pytest.mark.parametrize('dtype,n,rank,lda,ldk', K.STRIDED)
def test_pinv_with_leading_dimensions_above_the_order(rt, dtype, n, rank, lda, ldk):
    K.test_pinv_with_leading_dimensions_above_the_order(rt, dtype, n, rank, lda, ldk)


def test_fill_uniform(rt):
    K.test_fill_uniform_matches_oracle_hash(rt)


def test_errors(rt):
    K.test_errors_are_reported_not_thrown(rt)


@pytest.mark.parametrize('shape', [(1, 1, 1), (16, 16, 32), (130, 100, 70), (257, 128, 200), (100, 256, 129),
                                   (129, 300, 64), (3000, 256, 10000), (4097, 128, 6000), (5000, 64, 3000), (4097, 20, 200)])
def test_gemm_bf16_contraction(rt, shape):
    K.test_gemm_bf16_contraction(rt, shape)


@pytest.mark.parametrize('shape', [(1, 1, 1), (16, 16, 32), (100, 130, 70), (200, 257, 128), (129, 100, 256),
                                   (64, 129, 300), (300, 520, 100), (10000, 3000, 256), (6000, 4097, 128), (5000, 3000, 64), (200, 300, 40)])
def test_gemm_bf16_transposed_a(rt, shape):
    """Q = R^T G_i read from the row-major relation (ds_read_b64_tr_b16 fragments) on the hardware."""
    K.test_gemm_bf16_transposed_a(rt, shape)


@pytest.mark.parametrize('shape', [(1, 1, 1), (70, 100, 130), (128, 200, 257), (256, 129, 100), (300, 64, 129),
                                   (100, 300, 520), (256, 3000, 10000), (128, 6000, 4097), (64, 5000, 3000), (33, 260, 200)])
@pytest.mark.parametrize('transposed', [0, 1])
def test_gemm_bits_binary_relation_as_a_bitmap(rt, shape, transposed):
    K.test_gemm_bits_binary_relation_as_a_bitmap(rt, shape, transposed)


def test_binary_relations_as_bitmaps_in_the_engine():
    import test_emul_engine as E
    E.test_binary_relations_as_bitmaps_give_the_dense_results_bit_for_bit()
    E.test_fold_in_of_binary_new_relations_bf16()


@pytest.mark.parametrize('dtype,wide', [('f64', False), ('f64', True), ('bf16', False)])
def test_sparse_constraints_in_the_engine(dtype, wide):
    import test_emul_engine as E
    E.test_sparse_constraints_as_csr_give_the_dense_product(dtype, wide)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_sparse_constraints_at_8000_objects(dtype):
    """8000 x 8000 constraints (lambda I and 0.4 % similarity pairs of both signs, as config 5's) on a 6000 x 8000
    relation: CSR path (non-zero bound given) against the dense product on the same device-resident data."""
    import torch
    rs = np.random.RandomState(5)
    n, rank = {'u': 6000, 'm': 8000}, {'u': 40, 'm': 96}
    sim = np.where(rs.rand(8000, 8000) < 0.004, rs.randn(8000, 8000), 0.0)
    eye = 0.01 * np.eye(8000)
    R = rs.rand(6000, 8000)
    npd = np.float64 if dtype == 'f64' else np.float32
    mem = nat.get_runtime().mem
    out = {}
    for mode in ('sparse', 'dense'):
        thetas = []
        for T in (eye, sim):
            dm = DeviceMatrix(mem.from_host(np.ascontiguousarray(T, dtype=npd)), T.shape)
            dm.nnz = int(np.count_nonzero(T)) if mode == 'sparse' else 0
            thetas.append(('m', dm))
        plan = DevicePlan(['u', 'm'], n, rank, [('u', 'm', R, None)], thetas, nat.SKF_DFMF, dtype=dtype)
        for k, t in enumerate(['u', 'm']):
            plan.set_factor(t, fill_uniform((n[t], rank[t]), 100 + k, dtype))
        plan.iterate(5)
        out[mode] = [plan.get_factor(t) for t in ('u', 'm')]
        plan.close()
        del thetas
        torch.cuda.empty_cache()
    for a, b in zip(out['sparse'], out['dense']):
        # measured 5.7e-13 (f64) / 2.7e-7 (f32)
        within(relerr(a, b), 2.5e-12 if dtype == 'f64' else 1.2e-6, 'sparse vs dense constraints at 8000 objects, %s' % dtype)


def test_relation_pipeline_dfmf_and_dfmc_against_the_staged_schedule_and_the_oracle(monkeypatch):
    """Both iteration schedules on the hardware (two HIP streams, events between them): the relation pipeline of DFMF
    and of DFMC (completion between a masked relation's contractions) against SKF_NO_PIPELINE=1 and the oracle."""
    import test_emul_engine as E
    E.test_relation_pipelined_schedule_matches_the_staged_one_and_the_oracle(monkeypatch)
    monkeypatch.delenv('SKF_NO_PIPELINE', raising=False)
    E.test_dfmc_runs_the_relation_pipeline_with_the_completion_between_its_contractions(monkeypatch)


@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_round5_schedule_switches_keep_every_bit_on_the_hardware(dtype, monkeypatch):
    """Symmetric Gram launch, early update, chain products two to a launch: real streams, events and grids this time."""
    import test_emul_engine as E
    E.test_round5_schedule_switches_keep_every_bit(dtype, monkeypatch)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_gram_products_of_all_types_in_one_launch_on_the_hardware(dtype, monkeypatch):
    """Round 6: the grouped Gram launch on real grids (three products of different tile and slice counts in one grid)."""
    import test_emul_engine as E
    E.test_gram_products_of_all_types_in_one_launch_keep_every_bit(dtype, monkeypatch, three=True)


def _schedule_plans():
    import test_emul_engine as E
    return sorted(E.SCHEDULE_LAUNCHES)


@pytest.mark.parametrize('plan', _schedule_plans())
def test_launches_per_iteration_of_the_general_schedules_are_pinned_on_the_hardware(plan, monkeypatch):
    """The launch counts of the staged, pipelined and owned-rows schedules as measured before their steps were stated once
    (test_emul_engine.SCHEDULE_LAUNCHES), on real streams."""
    import test_emul_engine as E
    assert E.schedule_launches(plan, monkeypatch) == E.SCHEDULE_LAUNCHES[plan][-1], plan


def test_fit_with_a_rank_above_256_on_the_hardware(monkeypatch):
    """Orders 300 / 70 / 40 in one batch of step-per-launch sweeps inside a fit, and the Cholesky route, against the oracle."""
    import test_emul_engine as E
    E.test_fit_with_a_rank_above_256(monkeypatch)


def test_fit_with_a_rank_deficient_gram_above_order_256_on_the_hardware():
    """The multi-workgroup deflation inside a fit (round 6), against the oracle."""
    import test_emul_engine as E
    E.test_fit_with_a_rank_deficient_gram_above_order_256()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_fit_of_17_types_on_the_hardware(dtype, monkeypatch):
    """One type more than a pack / unpack launch of the pseudo-inverse holds, the declined matrix in the second chunk."""
    import test_emul_engine as E
    E.test_fit_of_17_types_packs_and_unpacks_in_chunks(dtype, monkeypatch)


def test_fit_with_every_rank_above_512_on_the_relation_pipeline():
    """Ranks above 512 leave the deep unsplit tile: the c x c products of the SECOND stream are cut into K slices while
    the main stream's split-K contractions are in flight -- each stream keeps its partials in its own scratch (round 6,
    advisor).  Two fits are bit-identical and match the oracle."""
    rs = np.random.RandomState(23)
    types = ['a', 'b', 'c']
    n = {'a': 1400, 'b': 1300, 'c': 1200}
    rank = {'a': 528, 'b': 520, 'c': 516}
    R = {('a', 'b'): [rs.rand(1400, 1300)], ('a', 'c'): [rs.rand(1400, 1200) - 0.3], ('b', 'c'): [rs.rand(1300, 1200)]}
    G0 = {(t, t): rs.rand(n[t], rank[t]) + 0.05 for t in types}
    Go, So = orc.dfmf(R, {}, types, rank, max_iter=2, G0=G0)
    fits = [_dfmf.dfmf(R, {}, types, rank, max_iter=2, G0=G0, dtype='f64') for _ in range(2)]
    for t in types:
        assert np.array_equal(fits[0][0][t, t], fits[1][0][t, t]), t
        within(relerr(fits[0][0][t, t], Go[t, t]), 1e-10, 'rank > 512: G')
    for k in So:
        assert np.array_equal(fits[0][1][k][0], fits[1][1][k][0]), k
        within(relerr(fits[0][1][k][0], So[k][0]), 1e-9, 'rank > 512: S')


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_two_runs_give_bit_identical_factors(dtype):
    """No float atomics and a fixed order for every sum (split-K slices, E / D contributions of the relations on the second
    stream, sum of B): two fits of the same plan inputs give bit-identical factors and backbones -- scaled config 5
    (DFMC on the relation pipeline: completion, bitmaps, CSR constraints, known-entry lists built with atomics whose
    order must not matter) and scaled config 3 (DFMF pipeline, split-K contractions)."""
    import torch
    import bench
    for c5 in (True, False):
        n = bench.sizes(0.12 if c5 else 0.1, bench.C5_FULL if c5 else None)
        out = []
        for rep in range(2):
            if c5:
                rels, thetas = bench.c5_graph(n, dtype)
                plan = DevicePlan(bench.C5_TYPES, n, bench.C5_RANKS, rels, thetas, nat.SKF_DFMC, dtype=dtype)
                types, ranks = bench.C5_TYPES, bench.C5_RANKS
            else:
                rels = [(i, j, bench.c3_relation(k, n, dtype), None) for k, (i, j, _) in enumerate(bench.PAIRS)]
                plan = DevicePlan(bench.TYPES, n, bench.RANKS, rels, [], nat.SKF_DFMF, dtype=dtype)
                types, ranks = bench.TYPES, bench.RANKS
            for k, t in enumerate(types):
                plan.set_factor(t, fill_uniform((n[t], ranks[t]), 100 + k, 'f32'))
            plan.iterate(4)
            out.append([plan.get_factor(t) for t in types] + [plan.get_backbone(k) for k in range(len(rels))])
            plan.close()
            del rels, plan
            torch.cuda.empty_cache()
        for a, b in zip(*out):
            np.testing.assert_array_equal(a, b)


def test_sparse_binary_relations_as_lists_on_the_hardware():
    """The list form of 0 / 1 relations (srp_bf16_v6_kernel<.., SRP_ONES>) at sizes where the lists are cut into parts pinned
    to XCDs: 3000 x 40000 at 1 % (row lists in 4 parts over 10 MB of bf16 factor rows) and 30000 x 3000 (column lists in 4
    parts over 15 MB), ranks 64 / 128 / 256 -- against host products of the bf16-rounded factors."""
    import test_emul_engine as E
    worst = E.sparse_binary_lists_case({'m': 3000, 'a': 40000, 'c': 30000}, {'m': 64, 'a': 128, 'c': 256}, 0.01, 35)
    # measured 0.0: the list kernel adds the same bf16-rounded rows in f32 in list order, as the host product does; the bound
    # leaves one f32 ulp per sum
    within(worst, 1.2e-7, 'sparse 0/1 relations as lists over bf16 factor rows: P, Q vs host products of the rounded factors')


def test_very_sparse_binary_relations_on_the_hardware():
    """The CSR / CSC gather path of 0 / 1 relations with at most 1 entry in 256 set: the emulator-suite case (ranks 8 / 12:
    binary_spmm_kernel over the f32 factor rows), and a 30000 x 20000 relation at 0.1 % (config 5's movie x actor at 1/2
    scale; ranks 256 / 128: the lists over the bf16 factor rows) whose P and Q must equal the products with the
    bf16-rounded factors -- what the bitmap kernels compute as well -- to f32 rounding."""
    import test_emul_engine as E
    E.test_very_sparse_binary_relation_is_contracted_by_row_gathers()
    import torch
    from skfusion_amd._engine import device_matrix_from_tensor as wrap
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    n, rank = {'m': 30000, 'a': 20000}, {'m': 256, 'a': 128}
    At = (torch.rand((30000, 20000), generator=gen, device='cuda') < 0.001)
    dm = wrap(At.to(torch.bfloat16).contiguous())
    dm.binary = True
    torch.cuda.synchronize()                       # the engine reads the tensor on its own stream
    plan = DevicePlan(['m', 'a'], n, rank, [('m', 'a', dm, None)], [], nat.SKF_DFMF, dtype='bf16')
    G0 = {t: fill_uniform((n[t], rank[t]), 7 + k, 'f32') for k, t in enumerate(['m', 'a'])}
    for t in ('m', 'a'):
        plan.set_factor(t, G0[t])
    rounded = lambda G: nat.from_bf16_bits(nat.to_bf16_bits(np.ascontiguousarray(G, dtype=np.float32))).astype(np.float64)
    Gm, Ga = rounded(plan.get_factor('m')), rounded(plan.get_factor('a'))
    plan.iterate(1)
    P, Q = plan.get_contraction(0, 0), plan.get_contraction(0, 1)
    plan.close()
    A = At.cpu().numpy()
    rows, cols = np.arange(0, 30000, 997), np.arange(0, 20000, 613)
    # measured 7.1e-8 / 8.3e-8 with f32 rows in round 2 (f32 sums of ~20 / ~30 rows)
    within(relerr(P[rows], A[rows].astype(np.float64) @ Ga), 2e-8, 'sparse binary relation 30000 x 20000: P rows vs the product with the bf16-rounded factor')
    within(relerr(Q[cols], A[:, cols].astype(np.float64).T @ Gm), 2e-8, 'sparse binary relation 30000 x 20000: Q rows vs the product with the bf16-rounded factor')


def test_to_bf16(rt):
    K.test_to_bf16_and_transpose(rt)


# ---- engine vs goldens of the reference ----------------------------------------------------------
@pytest.mark.parametrize('init', ['random', 'random_c', 'random_vcol'])
def test_c1_readme_100_iterations_f64(init):
    z = golden('c1_readme_dfmf.npz')
    R, types, rank = readme_graph()
    snaps = Snapshots((0, 1, 9, 99))
    G, S = _dfmf.dfmf(R, {}, types, rank, max_iter=100, callback=snaps,
                      G0=g0_from(z, init + '/', types), dtype='f64')
    bound = {'random': 2.5e-12, 'random_c': 8e-10, 'random_vcol': 1.5e-10}[init]          # measured 3.3e-13 / 7.8e-11 (2.2e-10 in round 2) / 3.6e-11
    within(compare_snapshots(z, init + '/', snaps.snap, bound), bound, 'c1 f64 %s: (G, S) at iterations 1/2/10/100 vs golden' % init)
    errs = orc.relation_errors(R, G, S)
    for (i, j), e in errs.items():
        assert relerr(e, z['%s/err_%s_%s' % (init, i, j)]) < 1e-9
    # device-resident loop without callback gives the same result
    G2, S2 = _dfmf.dfmf(R, {}, types, rank, max_iter=100, G0=g0_from(z, init + '/', types))
    for k in G:
        assert relerr(G2[k], G[k]) < 1e-12


@pytest.mark.parametrize('init', ['random', 'random_vcol', 'random_c'])
def test_c1_readme_f32_tolerances(init):
    """f32 engine (f32 relation contractions, f64 c x c algebra) vs the f64 oracle after 30
    iterations from the same G0: reconstruction error <= 1e-5 relative, G <= 1e-4, S <= 1e-3
    (Frobenius, relative) -- SURVEY.md 8d tolerances -- for every initialiser, including the
    ill-conditioned column-mean ones (cond(G^T G) ~ 1e4-1e5)."""
    z = golden('c1_readme_dfmf.npz')
    R, types, rank = readme_graph()
    G0 = g0_from(z, init + '/', types)
    G, S = _dfmf.dfmf(R, {}, types, rank, max_iter=30, G0=G0, dtype='f32')
    Go, So = orc.dfmf(R, {}, types, rank, max_iter=30, G0=G0)
    for t in types:
        assert relerr(G[t, t], Go[t, t]) < 1e-4
    for k in So:
        assert relerr(S[k][0], So[k][0]) < 1e-3
    e, eo = orc.relation_errors(R, G, S), orc.relation_errors(R, Go, So)
    for k in e:
        assert abs(e[k][0] - eo[k][0]) / eo[k][0] < 1e-5


def test_seeded_run_matches_reference_rng_stream():
    z = golden('c1_readme_dfmf.npz')
    R, types, rank = readme_graph()
    for init in ('random', 'random_c', 'random_vcol'):
        snaps = Snapshots((0, 99))
        _dfmf.dfmf(R, {}, types, rank, max_iter=100, init_type=init, callback=snaps,
                   random_state=np.random.RandomState(0))
        compare_snapshots(z, init + '/', snaps.snap, 1e-9)


def test_probe_graph_dfmf_and_dfmc():
    z = golden('probe_multirel.npz')
    R, Theta, M, types, rank = probe_graph(z)
    snaps = Snapshots((0, 1, 9, 29))
    _dfmf.dfmf(R, Theta, types, rank, max_iter=30, callback=snaps, G0=g0_from(z, 'dfmf/', types))
    compare_snapshots(z, 'dfmf/', snaps.snap, 1e-9)
    keep = {k: [m.copy() for m in v] for k, v in R.items()}
    snaps = Snapshots((0, 1, 9, 29))
    _dfmc.dfmc(R, M, Theta, types, rank, max_iter=30, callback=snaps, G0=g0_from(z, 'dfmc/', types))
    compare_snapshots(z, 'dfmc/', snaps.snap, 1e-9)
    for k in R:
        for a, b in zip(R[k], keep[k]):
            np.testing.assert_array_equal(a, b)
    # f32 engine on the same graph stays within the f32 tolerance of the f64 golden
    snaps = Snapshots((29,))
    _dfmc.dfmc(R, M, Theta, types, rank, max_iter=30, callback=snaps, G0=g0_from(z, 'dfmc/', types),
               dtype='f32')
    compare_snapshots(z, 'dfmc/', snaps.snap, 2e-3)


def test_c5_movielens_style_dfmc_f64_f32_bf16():
    """BASELINE config 5 (scaled, tests/helpers.py): f64 to 1e-9 of the reference golden over 30
    iterations; f32 / bf16 engines judged on the known-entry and held-out RMSE of the ratings."""
    from helpers import movielens_style_graph
    z = golden('c5_movielens_scaled.npz')
    R, M, Theta, types, rank = movielens_style_graph()
    G0 = g0_from(z, 'dfmc/', types)
    snaps = Snapshots((0, 1, 9, 29))
    _dfmc.dfmc(R, M, Theta, types, rank, max_iter=30, callback=snaps, G0=G0)
    within(compare_snapshots(z, 'dfmc/', snaps.snap, 1.5e-11), 1.5e-11, 'c5 scaled f64: (G, S) over 30 iterations vs golden')   # measured 3.3e-12
    known = ~M['user', 'movie'][0]
    # measured (round 4, MI355X): f32 2.7e-7 known / 1.1e-7 unknown, bf16 4.6e-4 known / 6.2e-7 unknown (the unknown entries
    # average the rounding of ~10^5 cells; round 2, before the known-entry lists: 1.0e-3 / 4.6e-4)
    for dtype, tol in (('f32', (1.2e-6, 1e-6)), ('bf16', (4.5e-3, 6e-6))):
        G, S = _dfmc.dfmc(R, M, Theta, types, rank, max_iter=30, G0=G0, dtype=dtype)
        d = G['user', 'user'].dot(S['user', 'movie'][0]).dot(G['movie', 'movie'].T) - R['user', 'movie'][0]
        for sel, key, bound in ((known, 'dfmc/rmse_known', tol[0]), (~known, 'dfmc/rmse_unknown', tol[1])):
            got = np.sqrt(np.mean(d[sel] ** 2))
            within(abs(got - float(z[key])) / float(z[key]), bound, 'c5 scaled %s: %s vs reference golden' % (dtype, key))


@pytest.mark.parametrize('variant', ['dfmf', 'dfmc'])
def test_rank_deficient_100_iterations(variant):
    z = golden('rank_deficient.npz')
    R, types, rank = rank_deficient_graph(z)
    G0 = g0_from(z, variant + '/', types)
    snaps = Snapshots((0, 1))
    if variant == 'dfmf':
        G, S = _dfmf.dfmf(R, {}, types, rank, max_iter=100, callback=snaps, G0=G0)
    else:
        G, S = _dfmc.dfmc(R, {k: [None] for k in R}, {}, types, rank, max_iter=100,
                          callback=snaps, G0=G0)
    within(compare_snapshots(z, variant + '/', snaps.snap, 1e-10), 1e-10, 'rank-deficient f64 %s: (G, S) vs golden' % variant)   # measured 9.1e-12
    assert all(np.isfinite(v).all() for v in G.values())
    errs = orc.relation_errors(R, G, S)
    for (i, j), e in errs.items():
        want = z['%s/err_%s_%s' % (variant, i, j)]
        assert abs(e[0] - want[0]) <= 1e-5 * max(1.0, want[0])


@pytest.mark.parametrize('init', ['random_c', 'random_vcol', 'random'])
def test_transform_fold_in(init):
    z = golden('transform_readme.npz')
    G = {(t, t): z['G_%s' % t] for t in TYPES}
    S = {('t1', 't2'): [z['S_t1_t2']], ('t1', 't3'): [z['S_t1_t3']], ('t2', 't1'): [z['S_t2_t1']]}
    Rn = {('t1', 't2'): [z['new_t1_t2']], ('t1', 't3'): [z['new_t1_t3']], ('t2', 't1'): [z['new_t2_t1']]}
    rank = {'t1': 10, 't2': 20, 't3': 30}
    snaps = {}
    Gi = _dfmf.transform(Rn, {('t1', 't1'): [z['theta_t1']]}, 't1', rank, G, S, max_iter=100,
                         init_type=init, random_state=np.random.RandomState(4),
                         callback=lambda g, it: snaps.__setitem__(it, g.copy()))
    for it in (0, 9, 99):
        assert relerr(snaps[it], z['%s/G_it%d' % (init, it)]) < 1e-9
    Gi32 = _dfmf.transform(Rn, {('t1', 't1'): [z['theta_t1']]}, 't1', rank, G, S, max_iter=100,
                           G0=z[init + '/G0'], dtype='f32')
    within(relerr(Gi32, z['%s/G_it99' % init]), 1e-5, 'fold-in f32 %s: G after 100 iterations vs golden' % init)
    Gib = _dfmf.transform(Rn, {('t1', 't1'): [z['theta_t1']]}, 't1', rank, G, S, max_iter=100,
                          G0=z[init + '/G0'], dtype='bf16')
    within(relerr(Gib, z['%s/G_it99' % init]), 1e-2, 'fold-in bf16 %s: G after 100 iterations vs golden' % init)   # measured 2.1e-3 (f32: 2.0e-6)


@pytest.mark.parametrize('schedule', ['fused', 'staged'])
def test_c2_dicty_dfmf_100_iterations_f64_and_f32(schedule, monkeypatch):
    """BASELINE config 2: dicty (2 relations + the ppi constraint), ranks 50/15/5.  fused: the
    job-table schedule for small graphs (skf_small.h, 9 launches per iteration); staged: the
    general schedule (SKF_NO_SMALL_FUSED=1)."""
    if schedule == 'staged':
        monkeypatch.setenv('SKF_NO_SMALL_FUSED', '1')
    z = golden('c2_dicty.npz')
    R, Theta, types, rank = dicty_graph()
    G0 = g0_from(z, 'dfmf/', types)
    snaps = Snapshots((0, 9, 99))
    G, S = _dfmf.dfmf(R, Theta, types, rank, max_iter=100, callback=snaps, G0=G0, dtype='f64')
    within(compare_snapshots(z, 'dfmf/', snaps.snap, 5e-9), 5e-9, 'dicty f64 dfmf: (G, S) at iterations 1/10/100 vs golden')   # measured 9.7e-10 (cond(G0^T G0) = 4e5)
    errs = orc.relation_errors(R, G, S)
    for (i, j), e in errs.items():
        assert relerr(e, z['dfmf/err_%s_%s' % (i, j)]) < 1e-9
    G32, S32 = _dfmf.dfmf(R, Theta, types, rank, max_iter=100, G0=G0, dtype='f32')
    e32 = orc.relation_errors(R, G32, S32)
    for k in errs:
        assert abs(e32[k][0] - errs[k][0]) / errs[k][0] < 1e-5
    for t in types:
        assert relerr(G32[t, t], G[t, t]) < 1e-3


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_batched_restarts_are_the_individual_runs(dtype):
    """skf_iterate_batch on the hardware: eight restarts of the dicty graph (sparse ppi constraint) share every launch;
    each plan ends with exactly the factors and backbones of its own skf_iterate run (bit for bit: the restart is a grid
    dimension, nothing else changes)."""
    from skfusion_amd._engine import flatten_relations, flatten_thetas, upload_graph
    R, Theta, types, rank = dicty_graph()
    n = {'gene': R['gene', 'go'][0].shape[0], 'go': R['gene', 'go'][0].shape[1], 'exc': R['gene', 'exc'][0].shape[1]}
    rel, thetas = upload_graph(flatten_relations(R), flatten_thetas(Theta), dtype)
    rs = np.random.RandomState(11)
    starts = [{t: rs.rand(n[t], rank[t]) + 0.01 for t in types} for _ in range(8)]

    def make(G0):
        plan = DevicePlan(types, n, rank, rel, thetas, nat.SKF_DFMF, dtype=dtype)
        for t in types:
            plan.set_factor(t, G0[t])
        return plan
    alone = []
    for G0 in starts:
        plan = make(G0)
        plan.iterate(20)
        alone.append(([plan.get_factor(t) for t in types], [plan.get_backbone(k) for k in range(len(rel))]))
        plan.close()
    plans = [make(G0) for G0 in starts]
    assert all(p.batchable() for p in plans) and DevicePlan.iterate_batch(plans, 20)
    for plan, (G, S) in zip(plans, alone):
        for t, g in zip(types, G):
            np.testing.assert_array_equal(plan.get_factor(t), g)
        for k, sk in enumerate(S):
            np.testing.assert_array_equal(plan.get_backbone(k), sk)
        plan.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_small_graph_schedule_on_an_awkward_graph(dtype, monkeypatch):
    """tests/small_cases.py: every job kind of skf_small.h on sizes that fit no tile (5 / 70 / 130 / 257 objects, ranks
    1 / 7 / 33 / 64, a multi-relation, several sparse constraints per type, empty rows); 10 iterations of the small-graph
    schedule vs the oracle and vs the general schedule."""
    import small_cases
    worst_o, worst_s = small_cases.check(dtype, monkeypatch, iters=10)
    # measured: f64 2.1e-13 / 2.4e-13, f32 1.1e-5 / 4.3e-6
    within(worst_o, 2e-12 if dtype == 'f64' else 1.1e-4, 'awkward small graph %s: small-graph schedule vs oracle, 10 iterations' % dtype)
    within(worst_s, 2.4e-12 if dtype == 'f64' else 4e-5, 'awkward small graph %s: small-graph vs general schedule' % dtype)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_device_squared_error_on_unaligned_shapes(dtype):
    """skf_relation_sqerr sizes one partial per workgroup of the tile the product runs on; dicty's shapes (1219 x 116,
    1219 x 282, ranks 50 / 15 / 5) take the small tile with run-time staging modes.  Device value vs host arithmetic."""
    from skfusion_amd._engine import DevicePlan, flatten_relations, flatten_thetas
    z = golden('c2_dicty.npz')
    R, Theta, types, rank = dicty_graph()
    G0 = g0_from(z, 'dfmf/', types)
    n = {'gene': R['gene', 'go'][0].shape[0], 'go': R['gene', 'go'][0].shape[1], 'exc': R['gene', 'exc'][0].shape[1]}
    rel = flatten_relations(R)
    plan = DevicePlan(types, n, rank, rel, flatten_thetas(Theta), nat.SKF_DFMF, dtype=dtype)
    for t in types:
        plan.set_factor(t, G0[t, t])
    plan.iterate(100)
    G = {t: plan.get_factor(t).astype(np.float64) for t in types}
    for k in range(len(rel)):
        i, j = rel[k][0], rel[k][1]
        host = np.linalg.norm(R[i, j][0] - G[i] @ plan.get_backbone(k).astype(np.float64) @ G[j].T)
        dev = float(np.sqrt(plan.relation_sqerr(k)))
        # measured: f64 2e-16 (one ulp; the bound is a rounding-level floor of 20 ulp), f32 1.6e-7
        within(abs(dev - host) / host, 5e-15 if dtype == 'f64' else 1.6e-6, 'dicty %s: device squared error vs host arithmetic' % dtype)
    # the error of the 100th iterate of the reference (golden): the fit itself, through the device's own error pass
    if dtype == 'f64':
        assert abs(np.sqrt(plan.relation_sqerr(0)) - float(np.ravel(z['dfmf/err_gene_go'])[0])) < 0.05
    plan.close()


def test_c2_dicty_dfmc_row_block_mask():
    z = golden('c2_dicty.npz')
    R, Theta, types, rank = dicty_graph()
    lo, hi = [int(v) for v in z['dfmc/mask_rows']]
    mask = np.zeros(R['gene', 'go'][0].shape, dtype=bool)
    mask[lo:hi] = True
    M = {('gene', 'go'): [mask], ('gene', 'exc'): [None]}
    snaps = Snapshots((0, 9, 29))
    G, S = _dfmc.dfmc(R, M, Theta, types, rank, max_iter=30, callback=snaps,
                      G0=g0_from(z, 'dfmf/', types))
    within(compare_snapshots(z, 'dfmc/', snaps.snap, 2.5e-9), 2.5e-9, 'dicty f64 dfmc: (G, S) vs golden')   # measured 5.7e-10
    assert relerr(G['gene', 'gene'][:256], z['dfmc/G_gene_final_rows']) < 1e-8


def test_c3_scaled_f64_and_f32():
    """1/25-linear-scale BASELINE config 3 (ranks 128/256/256): errors per iteration, S, G rows."""
    z = golden('c3_scaled.npz')
    R, G0, types, rank = c3_scaled_graph(z)
    errs = []

    def cb(G, S, it):
        e = orc.relation_errors(R, G, S)
        errs.append([e[k][0] for k in sorted(e)])
        for t in types:
            assert relerr(G[t, t][:16], z['Grows_%s_it%d' % (t, it)]) < 1e-8
    G, S = _dfmf.dfmf(R, {}, types, rank, max_iter=5, callback=cb, G0=G0, dtype='f64')
    assert relerr(np.array(errs), z['errs']) < 1e-9
    for (i, j) in R:
        assert relerr(S[i, j][0], z['S_%s_%s_it4' % (i, j)]) < 1e-7
    G32, S32 = _dfmf.dfmf(R, {}, types, rank, max_iter=5, G0=G0, dtype='f32')
    e32 = orc.relation_errors(R, G32, S32)
    want = z['errs'][4]
    got = [e32[k][0] for k in sorted(e32)]
    assert relerr(got, want) < 1e-5


def test_c3_planted_scaled_against_the_reference_golden():
    """The planted variant of config 3 at 1/25 linear scale (the one workload whose RMSE discriminates),
    inputs regenerated from the counter-based generator, against what the REFERENCE reached on them
    (tests/golden/c3_planted_scaled.npz: per-relation errors at iterations 10 / 30 / 60, backbones and factor rows at 60):
    f64 engine 1e-12; f32 engine RMSE within 4e-6; bf16 engine against the reference run on the bf16-rounded relations within
    5e-2 at this size (see the bounds below) -- and the device's planted generator (bench.c3_relation) forms the same relations as the host."""
    import torch
    import bench
    from helpers import c3_planted_graph
    z = golden('c3_planted_scaled.npz')
    keep = [int(v) for v in z['f64/iters']]
    R, G0, types, rank = c3_planted_graph()
    Rb = c3_planted_graph(bf16=True)[0]
    n = dict(zip(types, [int(v) for v in z['shape']]))
    cache = {}
    for k, (i, j, _) in enumerate(bench.PAIRS):
        dm = bench.c3_relation(k, n, 'f32', 'planted', cache)
        dev = dm.buf.owner.view(torch.float32).view(n[i], n[j]).cpu().numpy().astype(np.float64)
        within(relerr(dev, R[i, j][0]), 2e-6, 'planted generator on the device (f32) vs the host graph of the golden, relation %d' % k)
    # measured: f64 2.9e-14, f32 7.8e-7, bf16 3.7e-2 -- the bf16 engine also rounds the FACTOR operand of the two contractions
    # (P = R bf16(G_j), Q = R^T bf16(G_i)), which the reference on the rounded relations does not: at this size (1600 - 4000
    # objects per type) that adds 0.7 / 3.3 / 1.0 % to the three RMSEs (1.310 / 1.487 / 1.309 x the floor against 1.3005 /
    # 1.4392 / 1.2963); at full size it is below 0.5 % (tests/test_gpu_fullsize.py: RMSE_bf16^2 = RMSE_f32^2 + q^2 to 1.5 %)
    for dtype, tol_err, Rref, tag in (('f64', 1e-12, R, 'f64'), ('f32', 4e-6, R, 'f64'), ('bf16', 5e-2, Rb, 'bf16')):
        errs = {}

        def cb(G, S, it):
            if it in keep:
                e = orc.relation_errors(Rref, G, S)
                errs[it] = np.array([e[k][0] for k in sorted(e)])
                if it == keep[-1]:
                    errs['G'], errs['S'] = G, S
        _dfmf.dfmf(R, {}, types, rank, max_iter=keep[-1] + 1, G0=G0, dtype=dtype, callback=cb)
        worst = 0.0
        for q, it in enumerate(keep):
            dev = np.abs(errs[it] / z['%s/errs' % tag][q] - 1.0).max()
            worst = max(worst, dev)
            print('planted c3 at 1/25 scale, %s engine, iteration %d: relation errors vs the reference %.3e' % (dtype, it + 1, dev))
        within(worst, tol_err, 'planted c3 at 1/25 scale, %s engine: relation errors at iterations 10 / 30 / 60 vs the reference%s'
               % (dtype, ' on the bf16-rounded relations' if dtype == 'bf16' else ''))
        if dtype == 'f64':
            for t in types:
                within(relerr(errs['G'][t, t][:16], z['f64/Grows_%s' % t]), 2.5e-11, 'planted c3, f64: 16 rows of G_%s at iteration 60' % t)
            for (i, j) in R:
                within(relerr(errs['S'][i, j][0], z['f64/S_%s_%s' % (i, j)]), 2e-9, 'planted c3, f64: backbone %s-%s at iteration 60' % (i, j))


def test_accumulate_apply_split_equals_iterate():
    """skf_accumulate + skf_apply_update (the relation-sharded iteration, here on one device and
    without a process group) gives the same iterates as skf_iterate."""
    z = golden('probe_multirel.npz')
    R, Theta, M, types, rank = probe_graph(z)
    G0 = g0_from(z, 'dfmf/', types)
    G, S = _dfmf.dfmf(R, Theta, types, rank, max_iter=10, G0=G0, shard='relations')
    for t in types:
        assert relerr(G[t, t], z['dfmf/G_%s_it9' % t]) < 1e-9
    Gc, Sc = _dfmc.dfmc(R, M, Theta, types, rank, max_iter=10, G0=g0_from(z, 'dfmc/', types), shard='relations')
    for t in types:
        assert relerr(Gc[t, t], z['dfmc/G_%s_it9' % t]) < 1e-9


def test_row_block_sharding_c3_scaled_c5_and_probe(monkeypatch):
    """SURVEY.md 8e row blocks on the device: 2 / 3 / 4 simulated ranks (lockstep plans on this one
    GPU, exchange ranges summed where RCCL would all-reduce) against the reference goldens -- the
    scaled config 3 (f64 errors + S, f32, bf16), config 5 (MovieLens-style Dfmc) and the probe graph."""
    import test_emul_engine as E
    from helpers import fit_row_blocks, movielens_style_graph
    for variant in ('dfmf', 'dfmc'):
        E.test_row_block_sharding_matches_reference_golden(variant)
    E.test_row_block_sharding_bf16_and_abi_errors()
    z = golden('c3_scaled.npz')
    R, G0, types, rank = c3_scaled_graph(z)
    Rb = {k: [nat.from_bf16_bits(nat.to_bf16_bits(v[0])).astype(np.float64)] for k, v in R.items()}
    for size, dtype, tol in ((3, 'f64', 1e-9), (4, 'f32', 1e-5), (2, 'bf16', 1e-2)):
        for G, S in fit_row_blocks('dfmf', R, None, {}, types, rank, G0, 5, size, dtype=dtype):
            e = orc.relation_errors(Rb if dtype == 'bf16' else R, G, S)
            got = np.array([e[k][0] for k in sorted(e)])
            assert np.abs(got - z['errs'][4]).max() / z['errs'][4].min() < tol, (size, dtype)
            if dtype == 'f64':
                for (i, j) in R:
                    assert relerr(S[i, j][0], z['S_%s_%s_it4' % (i, j)]) < 1e-7
    z5 = golden('c5_movielens_scaled.npz')
    R, M, Theta, types, rank = movielens_style_graph()
    for G, S in fit_row_blocks('dfmc', R, M, Theta, types, rank, g0_from(z5, 'dfmc/', types), 30, 4):
        for t in types:
            assert relerr(G[t, t], z5['dfmc/G_%s_it29' % t]) < 1e-9
        for (i, j) in R:
            assert relerr(S[i, j][0], z5['dfmc/S_%s_%s_0_it29' % (i, j)]) < 1e-9
    # the bf16 engine under row blocks (bitmaps, CSR / CSC of the sparse 0 / 1 relations and the completion lists are built
    # per block): against the same engine on whole relations
    # (both on the dense path with its completed bf16 copy -- plans with row blocks always take it; by default the whole
    # ratings relation would be kept as lists of its known entries, which do not round completed entries to bf16)
    G0 = g0_from(z5, 'dfmc/', types)
    monkeypatch.setenv('SKF_DFMC_SPARSE', '0')
    Gw, Sw = _dfmc.dfmc(R, M, Theta, types, rank, max_iter=5, G0=G0, dtype='bf16')
    monkeypatch.delenv('SKF_DFMC_SPARSE')
    for G, S in fit_row_blocks('dfmc', R, M, Theta, types, rank, G0, 5, 3, dtype='bf16'):
        for t in types:
            within(relerr(G[t, t], Gw[t, t]), 2e-3, 'c5 scaled bf16, 3 row blocks vs whole relations: G_%s after 5 iterations' % t)


def test_owned_rows_random_graphs(rt):
    """tools/fuzz_owned.py: random graphs (1 .. 700 objects, ranks on both sides of 64, multi-relations, masks of every
    density, sparse and dense constraints, 2 .. 4 ranks) through the ownership-sharded fit, every engine against the oracle
    and against what ONE device deviates by on the same graph."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import fuzz_owned
    assert fuzz_owned.fuzz(10, 5, 3) == 0


def test_owned_rows_sharding_on_the_device(rt, monkeypatch):
    """SKF_OPT_OWNED_ROWS on the hardware: the ranks of a group as threads of this process on ONE GPU (helpers.ThreadGroup),
    every plan driving skf_iterate_dist with its three streams (contractions / chains and side products / exchanges) -- the
    probe and config-5 goldens over 2 and 3 ranks (1e-9), the wide-rank graph in all three engines, the ABI errors, the
    byte accounting of config 3 on 8 ranks; then the scaled config 3 over 4 ranks in f64 / f32 / bf16 against the golden's
    reconstruction errors, with the exchanges on the main stream as well (SKF_COMM_STREAM=0: same results)."""
    import test_owned_sharding as O
    from helpers import fit_owned
    for variant in ('dfmf', 'dfmc'):
        O.test_owned_rows_reproduce_the_reference_golden_on_2_and_3_ranks(variant)
        O.test_owned_rows_wide_ranks_all_engines(variant)
    O.test_owned_rows_c5_movielens_style_dfmc()
    O.test_owned_rows_dense_constraint_in_the_bf16_engine()
    O.test_owned_rows_rank_deficient_gram()
    for variant in ('dfmf', 'dfmc'):
        O.test_owned_rows_mixed_ranks(variant)
    for dtype, ranks, tol in (('f64', {'a': 16, 'b': 12, 'c': 8}, 1e-9), ('bf16', {'a': 128, 'b': 64, 'c': 16}, 2e-2)):
        O.test_owned_rows_keep_the_lists_of_known_entries(dtype, ranks, tol, monkeypatch)
    monkeypatch.delenv('SKF_DFMC_SPARSE', raising=False)
    O.test_exchange_bytes_of_config_3_on_8_ranks(rt)
    O.test_owned_rows_abi_errors(rt)
    z = golden('c3_scaled.npz')
    R, G0, types, rank = c3_scaled_graph(z)
    Rb = {k: [nat.from_bf16_bits(nat.to_bf16_bits(v[0])).astype(np.float64)] for k, v in R.items()}
    # measured: f64 5.1e-15, f32 1.5e-9, bf16 1.4e-5 / 1.6e-5 (the sharded fit deviates by what the single device does)
    for size, dtype, tol, comm_stream in ((3, 'f64', 5e-14, '1'), (4, 'f32', 1.5e-8, '1'), (4, 'bf16', 1.5e-4, '1'), (2, 'bf16', 1.5e-4, '0')):
        monkeypatch.setenv('SKF_COMM_STREAM', comm_stream)
        out, grp, said = fit_owned('dfmf', R, None, {}, types, rank, G0, 5, size, dtype=dtype)
        for G, S in out:
            e = orc.relation_errors(Rb if dtype == 'bf16' else R, G, S)
            got = np.array([e[k][0] for k in sorted(e)])
            within(np.abs(got - z['errs'][4]).max() / z['errs'][4].min(), tol,
                   'c3 scaled, %d owned-row ranks, %s: reconstruction errors after 5 iterations vs the golden' % (size, dtype))
            if dtype == 'f64':
                for (i, j) in R:
                    assert relerr(S[i, j][0], z['S_%s_%s_it4' % (i, j)]) < 1e-7
        for t in types:
            for G, _ in out[1:]:
                np.testing.assert_array_equal(G[t, t], out[0][0][t, t])
        # per iteration what skf_exchange_bytes says; bf16: plus ONE gather of the f32 rows at the end of the call
        final = (size - 1) / float(size) * sum(O.owned_rows(dtype, G0[t, t].shape[0], 0, size)[2] * size * rank[t] * 4
                                               for t in types) if dtype == 'bf16' else 0.0
        assert abs(grp.bytes_sent_per_rank() - 5 * said[0] - final) <= 5.0
    monkeypatch.delenv('SKF_COMM_STREAM')


def test_rccl_stream_ordered_exchanges_single_rank(monkeypatch):
    """The RCCL path of the sharded iterations (collectives issued on the engine's stream, no host
    synchronisation between the stages) with a one-rank nccl group on this box's GPU: the all-reduces
    are identities, the iterates must equal the golden.  (Real multi-rank runs: gloo tests on CPU,
    the driver's multi-GPU bench.)"""
    import socket
    import torch
    import torch.distributed as dist
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    try:
        dist.init_process_group('nccl', init_method='tcp://127.0.0.1:%d' % port, rank=0, world_size=1,
                                device_id=torch.device('cuda', torch.cuda.current_device()))
    except Exception as exc:                                  # pragma: no cover
        pytest.skip('no one-rank RCCL group on this box: %r' % (exc,))
    try:
        monkeypatch.setenv('SKF_FORCE_COLLECTIVES', '1')
        z = golden('probe_multirel.npz')
        R, Theta, M, types, rank = probe_graph(z)
        for shard in ('relations', 'rows', 'owned'):
            G, S = _dfmf.dfmf(R, Theta, types, rank, max_iter=10, G0=g0_from(z, 'dfmf/', types), shard=shard)
            for t in types:
                assert relerr(G[t, t], z['dfmf/G_%s_it9' % t]) < 1e-9
            Gc, Sc = _dfmc.dfmc(R, M, Theta, types, rank, max_iter=10, G0=g0_from(z, 'dfmc/', types), shard=shard)
            for t in types:
                assert relerr(Gc[t, t], z['dfmc/G_%s_it9' % t]) < 1e-9
        # the exchanges of those fits were issued by the library on its own RCCL communicator (skf_comm_unique_id /
        # skf_comm_create / skf_iterate_dist): reduce-scatter of E and D, update of the owned range, all-gather of G.  On a
        # scaled config 3 in bf16 the same path must equal the staged single-device iteration bit for bit.
        import bench
        monkeypatch.setenv('SKF_NO_PIPELINE', '1')
        n = bench.sizes(0.05)
        out = []
        for use_library in (True, False):
            rels = [(i, j, bench.c3_relation(k, n, 'bf16'), None) for k, (i, j, _) in enumerate(bench.PAIRS)]
            plan = DevicePlan(bench.TYPES, n, bench.RANKS, rels, [], nat.SKF_DFMF, dtype='bf16')
            for k, t in enumerate(bench.TYPES):
                plan.set_factor(t, fill_uniform((n[t], bench.RANKS[t]), 100 + k, 'f32'))
            if use_library:
                assert plan.attach_comm()
                assert plan.exchange_bytes(8) >= 3 * 7 / 8 * sum(n[t] * bench.RANKS[t] * 4 for t in bench.TYPES)
                plan.iterate_dist(3)
            else:
                plan.iterate(3)
            out.append([plan.get_factor(t) for t in bench.TYPES])
            plan.close()
        for a, b in zip(*out):
            np.testing.assert_array_equal(a, b)
        # ownership-sharded plan of the ONE rank (reduce-scatter of Q, all-gather of the bf16 rows as bytes, all-reduce of the
        # c x c sums -- all in place through RCCL, exchanges on their own stream): the same iteration up to the order in which
        # the type term joins E / D (a launch of its own here, fused into the last side product there)
        from skfusion_amd._engine import owned_rows
        rels = []
        for k, (i, j, _) in enumerate(bench.PAIRS):
            a, cnt, _ = owned_rows('bf16', n[i], 0, 1)
            assert (a, cnt) == (0, n[i])
            rels.append((i, j, bench.c3_relation(k, n, 'bf16'), None, dict(absent=False, row_begin=0, n_rows=cnt, masked=False)))
        plan = DevicePlan(bench.TYPES, n, bench.RANKS, rels, [], nat.SKF_DFMF, dtype='bf16', part=(0, 1), owned=True)
        for k, t in enumerate(bench.TYPES):
            plan.set_factor(t, fill_uniform((n[t], bench.RANKS[t]), 100 + k, 'f32'))
        assert plan.attach_comm()
        plan.iterate_dist(3)
        for t, b in zip(bench.TYPES, out[1]):
            # measured 7.0e-5 on the smallest type (rank 256 over 2000 objects: the backbones amplify the reordered f32 sums)
            within(relerr(plan.get_factor(t), b), 3.5e-4, 'one-rank RCCL, owned rows, bf16 c3 at 1/20 scale: G_%s vs the staged iteration' % t)
        plan.close()
    finally:
        dist.destroy_process_group()


def test_config5_at_scale_bf16_engine_tracks_f32_engine():
    """BASELINE config 5 at 1/5 linear scale (20k users x 8k movies, ranks 128/256/16/128/64/64, 98 % of
    the ratings unknown, two constraints): the bf16 engine (bf16 completion kernel, bf16 constraint
    halves, 256-row contraction tiles with several column tiles) against the f32 engine on the same
    device-resident data -- per-relation RMSE after 6 iterations within 2 %, everything finite."""
    import torch
    import bench
    n = bench.sizes(0.2, bench.C5_FULL)
    rm = {}
    for dtype in ('f32', 'bf16'):
        rels, thetas = bench.c5_graph(n, dtype)
        plan = DevicePlan(bench.C5_TYPES, n, bench.C5_RANKS, rels, thetas, nat.SKF_DFMC, dtype=dtype)
        for k, t in enumerate(bench.C5_TYPES):
            plan.set_factor(t, fill_uniform((n[t], bench.C5_RANKS[t]), 100 + k, 'f32'))
        plan.iterate(6)
        rm[dtype] = [np.sqrt(plan.relation_sqerr(k) / (n[i] * n[j])) for k, (i, j, _, _) in enumerate(bench.C5_PAIRS)]
        G = plan.get_factor('movie')
        assert np.isfinite(G).all() and (G >= 0).all()
        plan.close()
        del rels, thetas
        torch.cuda.empty_cache()
    for a, b in zip(rm['bf16'], rm['f32']):
        assert abs(a - b) <= 2e-2 * b, (rm['bf16'], rm['f32'])


def test_graph_replay_matches_golden(monkeypatch):
    """SKF_GRAPH=1: iterations 2..n of skf_iterate replay one captured hipGraph (opt-in; a capture
    failure falls back to eager launches): same iterates as the golden either way."""
    monkeypatch.setenv('SKF_GRAPH', '1')
    z = golden('probe_multirel.npz')
    R, Theta, M, types, rank = probe_graph(z)
    G, S = _dfmf.dfmf(R, Theta, types, rank, max_iter=30, G0=g0_from(z, 'dfmf/', types))
    for t in types:
        assert relerr(G[t, t], z['dfmf/G_%s_it29' % t]) < 1e-9
    Gc, Sc = _dfmc.dfmc(R, M, Theta, types, rank, max_iter=30, G0=g0_from(z, 'dfmc/', types), dtype='bf16')
    for t in types:
        assert np.isfinite(Gc[t, t]).all()


def test_bf16_completion_kernel_and_residual_pass():
    import test_emul_engine as E
    for known in (0.6, 0.04):
        E.test_bf16_completion_kernel_against_f32_engine(known)
    E.test_relation_sqerr_counts_the_partials_of_the_tile_it_launches()


def test_bf16_engine_c1_and_c3_scaled():
    """SKF_BF16 engine: bf16 relation contractions.  Tolerances: reconstruction
    error within 1e-2 relative of the f64 oracle on the same (bf16-rounded) relations."""
    import test_emul_engine as E
    E.test_bf16_engine_against_oracle_on_bf16_rounded_relations()
    E.test_bf16_dfmc_masked_completion()
    E.test_bf16_engine_odd_sizes_and_wide_rank()
    z = golden('c3_scaled.npz')
    R, G0, types, rank = c3_scaled_graph(z)
    G, S = _dfmf.dfmf(R, {}, types, rank, max_iter=5, G0=G0, dtype='bf16')
    Rb = {k: [nat.from_bf16_bits(nat.to_bf16_bits(v[0])).astype(np.float64)] for k, v in R.items()}
    e = orc.relation_errors(Rb, G, S)
    got = np.array([e[k][0] for k in sorted(e)])
    within(np.abs(got - z['errs'][4]).max() / z['errs'][4].min(), 7e-5, 'c3 scaled bf16: reconstruction error vs f64 golden')   # measured 1.4e-5
    Gf, Sf = _dfmf.dfmf(R, {}, types, rank, max_iter=5, G0=G0, dtype='f32')
    for t in types:
        bound = {'t1': 8e-4, 't2': 4e-3, 't3': 1.4e-2}[str(t)]        # measured 1.4e-4 / 1.6e-3 / 1.5e-3 (round 2: 1.7e-4 / 8.8e-4 / 4.4e-3)
        within(relerr(G[t, t], Gf[t, t]), bound, 'c3 scaled bf16: G_%s vs the f32 engine after 5 iterations' % t)


def test_device_side_error_and_generated_data_match_oracle(rt):
    """fill_uniform data + relation_sqerr on the device == the same graph built on the host."""
    n = {'t1': 300, 't2': 500, 't3': 200}
    rank = {'t1': 16, 't2': 32, 't3': 24}
    rels = [('t1', 't2', fill_uniform((300, 500), 0, 'f64'), None),
            ('t1', 't3', fill_uniform((300, 200), 1, 'f64'), None),
            ('t2', 't3', fill_uniform((500, 200), 2, 'f64'), None)]
    plan = DevicePlan(TYPES, n, rank, rels, [], nat.SKF_DFMF, dtype='f64')
    G0 = {}
    for k, t in enumerate(TYPES):
        plan.set_factor(t, fill_uniform((n[t], rank[t]), 100 + k, 'f64'))
        G0[t, t] = orc.hash_uniform_matrix(100 + k, n[t], rank[t])
    plan.iterate(8)
    R = {('t1', 't2'): [orc.hash_uniform_matrix(0, 300, 500)],
         ('t1', 't3'): [orc.hash_uniform_matrix(1, 300, 200)],
         ('t2', 't3'): [orc.hash_uniform_matrix(2, 500, 200)]}
    Go, So = orc.dfmf(R, {}, TYPES, rank, max_iter=8, G0=G0)
    for t in TYPES:
        assert relerr(plan.get_factor(t), Go[t, t]) < 1e-9
    eo = orc.relation_errors(R, Go, So)
    for k, (i, j, _, _) in enumerate(rels):
        assert abs(np.sqrt(plan.relation_sqerr(k)) - eo[i, j][0]) < 1e-9 * eo[i, j][0]
    plan.close()


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_full_size_properties_c3(rt, dtype):
    """BASELINE config 3 at FULL size (50k x 100k / 50k x 40k / 100k x 40k, ranks 128/256/256,
    f32 and bf16 engines): size-independent properties -- factors stay finite and non-negative, the summed
    reconstruction error does not increase over iterations (DFMF objective), and the RMSE sits
    at the iid-uniform floor sqrt(1/12) within 1%."""
    import torch
    if torch.cuda.get_device_properties(0).total_memory < 120e9:
        pytest.skip('needs > 120 GB of HBM')
    n = {'t1': 50000, 't2': 100000, 't3': 40000}
    rank = {'t1': 128, 't2': 256, 't3': 256}
    rels = [('t1', 't2', fill_uniform((n['t1'], n['t2']), 0, dtype), None),
            ('t1', 't3', fill_uniform((n['t1'], n['t3']), 1, dtype), None),
            ('t2', 't3', fill_uniform((n['t2'], n['t3']), 2, dtype), None)]
    plan = DevicePlan(TYPES, n, rank, rels, [], nat.SKF_DFMF, dtype=dtype)
    del rels[:]
    rels = [('t1', 't2'), ('t1', 't3'), ('t2', 't3')]
    for k, t in enumerate(TYPES):
        plan.set_factor(t, fill_uniform((n[t], rank[t]), 100 + k, 'f32'))
    prev = None
    for it in range(4):
        plan.iterate(1)
        tot = sum(np.sqrt(plan.relation_sqerr(k)) for k in range(3))
        assert np.isfinite(tot)
        if prev is not None:
            assert tot <= prev * (1 + (1e-6 if dtype == 'f32' else 1e-4))
        prev = tot
    for k, (i, j) in enumerate(rels):
        rmse = np.sqrt(plan.relation_sqerr(k) / (n[i] * n[j]))
        assert abs(rmse - np.sqrt(1 / 12.)) < 0.01 * np.sqrt(1 / 12.)
    G1 = plan.get_factor('t1')
    assert np.isfinite(G1).all() and (G1 >= 0).all()
    plan.close()


def test_rank_deficient_fit_at_rank_256_keeps_its_speed(rt):
    """A Gram matrix of order 256 that the Cholesky fast path rejects (half of the latent columns duplicated: the
    duplicates stay identical under the multiplicative updates, so EVERY iteration meets a rank-128 Gram matrix) goes
    through the rank-revealing deflation (4.0 ms, on the second stream under the contractions), not the one-workgroup
    Jacobi solver (216 ms per call in round 1): the rank-deficient fit sustains more than half of the full-rank
    iteration rate on a 30000 x 20000 relation, and on a small graph its factors are those of the f64 oracle with
    scipy's pseudo-inverse."""
    import time
    import torch
    types, rank = ['a', 'b'], {'a': 256, 'b': 128}
    n = {'a': 30000, 'b': 20000}
    rels = [('a', 'b', fill_uniform((n['a'], n['b']), 5, 'f32'), None)]
    rate = {}
    for name in ('full', 'deficient'):
        plan = DevicePlan(types, n, rank, rels, [], nat.SKF_DFMF, dtype='f32')
        for k, t in enumerate(types):
            g0 = orc.hash_uniform_matrix(40 + k, n[t], rank[t]) + 0.05
            if name == 'deficient' and t == 'a':
                g0[:, 128:] = g0[:, :128]
            plan.set_factor(t, g0)
        plan.iterate(2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan.iterate(6)
        torch.cuda.synchronize()
        rate[name] = 6 / (time.perf_counter() - t0)
        plan.close()
    within(rate['full'] / rate['deficient'], 2.0, 'rank-deficient fit at rank 256 (30000 x 20000, f32): full-rank it/s over deficient it/s')
    # parity of the deflated pseudo-inverse inside a fit (small graph, f64)
    rs = np.random.RandomState(12)
    n = {'a': 6000, 'b': 4000}
    Rm = rs.rand(6000, 4000)
    G0d = {t: rs.rand(n[t], rank[t]) + 0.05 for t in types}
    G0d['a'][:, 128:] = G0d['a'][:, :128]
    plan = DevicePlan(types, n, rank, [('a', 'b', Rm, None)], [], nat.SKF_DFMF, dtype='f64')
    for t in types:
        plan.set_factor(t, G0d[t])
    plan.iterate(8)
    Gd = {t: plan.get_factor(t) for t in types}
    plan.close()
    assert np.abs(Gd['a'][:, 128:] - Gd['a'][:, :128]).max() < 1e-9 * np.abs(Gd['a']).max()
    Go, So = orc.dfmf({('a', 'b'): [Rm]}, {}, types, rank, max_iter=8, G0={(t, t): G0d[t] for t in types})
    for t in types:
        bound = {'a': 2.5e-13, 'b': 1e-12}[str(t)]                 # measured 4.7e-14 / 1.9e-13
        within(relerr(Gd[t], Go[t, t]), bound, 'rank-deficient fit at rank 256: G_%s vs the oracle (scipy pinv) after 8 iterations' % t)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
@pytest.mark.parametrize('rank_a', [64, 128, 256])
def test_dfmc_on_the_known_entries_only_matches_the_dense_completion(dtype, rank_a, monkeypatch):
    """skf_relation_desc.known_bound on the hardware: a 3000 x 2600 masked relation with 2 % of its entries known kept as lists
    (csrc/skf_known.h; the relation-pipelined DFMC schedule) against the dense path with its completed copy -- (G, S), the
    squared errors of every iteration (skf_relation_sqerr: trace terms + one list pass), the row-side product and Q.  The
    ranks walk the list kernels: bf16 8 / 16 / 32 lanes per vector (v_dot2c + DPP), f32 16 / 32 / 64, f64 32 / 64 / any-width."""
    import known_cases as K
    n, ranks = {'a': 3000, 'b': 2600, 'c': 500}, {'a': rank_a, 'b': 256 if rank_a < 256 else 128, 'c': 64}
    # (G, S, squared errors, P S^T, Q), measured in round 3 (profiles/r03_test_deviations.txt):
    #   f64  3.6e-13 / 1.2e-12 / 2.6e-14 / 5.1e-13 / 7.6e-13      f32  1.4e-6 / 7.1e-6 / 3.0e-8 / 2.0e-6 / 4.7e-7
    #   bf16 2.3e-3 / 5.3e-3 / 1.1e-4 / 1.0e-2 / 2.3e-3  (the dense path rounds every completed entry to bf16, the lists do not)
    tol = {'f64': (1.5e-12, 6e-12, 1.3e-13, 2.5e-12, 4e-12), 'f32': (7e-6, 3.5e-5, 1.5e-7, 1e-5, 2.5e-6),
           'bf16': (1.2e-2, 2.5e-2, 5.5e-4, 5e-2, 1.2e-2)}[dtype]
    K.sparse_against_dense(n, ranks, 0.02, 4, dtype, tol, 'GPU %s rank %d' % (dtype, rank_a), monkeypatch)


@pytest.mark.parametrize('rank_a,parts,share', [(128, 2, 0.1), (128, 8, 0.1), (256, 4, 0.05), (128, 4, 0.2)])
def test_known_entry_lists_in_parts_on_the_v6_kernel(rank_a, parts, share, monkeypatch):
    """srp_bf16_v6_kernel (bf16, ranks 128 / 256 on the row type) with the lists cut into parts pinned to XCDs -- segments
    of a few full batches plus a tail (2 parts at 10 % known: 130 entries), tail-only segments (8 parts: 32), long ones
    (20 % known), the zero row behind the gathered matrix for every slot past a segment's end -- against the dense path."""
    import known_cases as K
    n, ranks = {'a': 3000, 'b': 2600, 'c': 500}, {'a': rank_a, 'b': 256 if rank_a < 256 else 128, 'c': 64}
    tol = (1.2e-2, 2.5e-2, 5.5e-4, 5e-2, 1.2e-2)
    K.sparse_against_dense(n, ranks, share, 4, 'bf16', tol, 'GPU bf16 rank %d parts %d known %.2f' % (rank_a, parts, share),
                           monkeypatch, parts, seed=parts)
