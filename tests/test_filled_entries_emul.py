"""Relations with missing values as entries plus rank one (SKF_REL_FILL_RANK1) on the host emulator: the passes, the error
pass and the refusals through DevicePlan, whole fits against the oracle on the expanded filled matrix, the public API."""
import numpy as np
import pytest

import skfusion_amd._native as nat
from emul.runtime import emulated_runtime, use_runtime

import filled_entries_cases as FC

N_A, N_B = 203, 197
N = {'a': 150, 'b': 130, 'c': 40}
RANKS = {'a': 20, 'b': 24, 'c': 5}


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


# (engine, rank of a, rank of b): a 16-byte-multiple width per engine and the scalar path of the column sums (5 and 15, the
# dicty ranks; bf16: ldrow = 8 / 16 != c)
VARIANTS = [('f64', 16, 32), ('f64', 5, 15), ('f32', 32, 16), ('f32', 15, 5), ('bf16', 64, 128), ('bf16', 5, 15)]


@pytest.mark.parametrize('parts', [1, 2, 4, 8])
@pytest.mark.parametrize('dtype,rank_a,rank_b', VARIANTS)
def test_passes_and_error_pass_against_host(dtype, rank_a, rank_b, parts, monkeypatch):
    pattern = ('edges', 'full', 'heavy')[(parts + rank_a) % 3]
    FC.pass_case(N_A, N_B, rank_a, rank_b, dtype, parts, pattern,
                 'emulator %s ranks %d/%d parts %d %s' % (dtype, rank_a, rank_b, parts, pattern), monkeypatch, seed=parts,
                 lengths=(1, 4, 5, 16, 17, 64, 65))


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_column_type_smaller_than_one_slab(dtype, monkeypatch):
    """n_j below the rows of one first-stage workgroup of the column sums, n_i on one full slab plus a tail."""
    assert 100 < FC.COLSUM_ROWS < 150
    FC.pass_case(150, 100, 16, 8, dtype, 1, 'full', 'emulator %s n_j < slab' % dtype, monkeypatch)


def test_flag_is_refused_where_it_does_not_apply():
    FC.refused_flag_cases()


@pytest.mark.parametrize('kind', ['missing', 'nan'])
@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_refused_at_bind(kind, dtype):
    FC.refused_at_bind_case(kind, dtype)


@pytest.mark.parametrize('fill', FC.FILLS)
def test_f64_fit_against_the_oracle_on_the_filled_matrix(fill):
    """G, S and the per-relation errors to 1e-9 after 10 iterations (the bound sparse_dfmf_cases.csr_against_oracle holds)."""
    FC.fit_against_oracle(N, RANKS, fill, 'f64', FC.fit_tol('f64'), 'emulator fill %r' % (fill,))


# f32 / bf16 against the f64 oracle: the emulator's own bounds (filled_entries_cases.FIT_TOL_EMUL; FIT_TOL is the hardware's)
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_f32_bf16_fit_against_the_f64_oracle(dtype):
    FC.fit_against_oracle(N, RANKS, 'row_mean', dtype, FC.FIT_TOL_EMUL[dtype], 'emulator %s' % dtype)


def test_dfmc_row_mean_against_the_dfmc_oracle_and_repeatable():
    FC.fit_against_oracle(N, RANKS, 'row_mean', 'f64', FC.fit_tol('f64'), 'emulator DFMC', variant=nat.SKF_DFMC)
    FC.dfmc_repeat_case(N, RANKS)


@pytest.mark.parametrize('fill', FC.FILLS)
def test_api_dfmf_never_expands(fill, monkeypatch):
    """Fails without the feature: Dfmf expands an unstored='unknown' relation to its MaskedArray."""
    FC.api_case(FC.Dfmf, fill, 'f64', (60, 50), monkeypatch)


def test_api_dfmc_line_means_never_expand(monkeypatch):
    FC.api_case(FC.Dfmc, 'col_mean', 'f64', (60, 50), monkeypatch)


def test_api_everything_else(tmp_path, monkeypatch):
    FC.api_everything_else_case((60, 50), 'f64', tmp_path, monkeypatch)
