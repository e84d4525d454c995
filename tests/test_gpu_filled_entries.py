"""Relations with missing values as entries plus rank one (SKF_REL_FILL_RANK1) on the MI355X: the lists, both passes and the
error pass against the host at the widths of the column-sum kernel's vector and scalar paths, the refusals, whole fits of
every engine against the f64 oracle on the expanded filled matrix, and the public API with every expansion forbidden."""
import numpy as np
import pytest

import skfusion_amd._native as nat

import filled_entries_cases as FC

pytestmark = pytest.mark.gpu

N_A, N_B = 459, 453         # the first stage of the column sums: 3 workgroups of COLSUM_ROWS = 128 rows and a tail of 75 / 69


@pytest.fixture(scope='module', autouse=True)
def no_clamps():
    from skfusion_amd._engine import split_clamps
    before = split_clamps()
    yield
    assert split_clamps() - before == 0


# (engine, rank of a = width of s = G_i^T a, rank of b = width of t = G_j^T b): a 16-byte-multiple width per engine (f64: 2,
# f32: 4, bf16: 8 elements) and the scalar path -- 5 and 15, the dicty ranks, and 20 on bf16 rows (ldrow = 24 != c)
VARIANTS = [('f64', 16, 128), ('f64', 5, 15), ('f32', 128, 24), ('f32', 15, 5), ('bf16', 128, 256), ('bf16', 5, 15),
            ('bf16', 20, 64)]


@pytest.mark.parametrize('parts', [1, 2, 4, 8])
@pytest.mark.parametrize('dtype,rank_a,rank_b', VARIANTS)
def test_lists_passes_and_error_pass_against_host(dtype, rank_a, rank_b, parts, monkeypatch):
    assert N_A // FC.COLSUM_ROWS >= 3 and N_A % FC.COLSUM_ROWS and N_B // FC.COLSUM_ROWS >= 3 and N_B % FC.COLSUM_ROWS
    for pattern in ('edges', 'full', 'heavy'):
        FC.pass_case(N_A, N_B, rank_a, rank_b, dtype, parts, pattern,
                     'GPU %s ranks %d/%d parts %d %s' % (dtype, rank_a, rank_b, parts, pattern), monkeypatch, seed=parts)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_column_type_smaller_than_one_slab(dtype, monkeypatch):
    assert 100 < FC.COLSUM_ROWS
    FC.pass_case(N_A, 100, 16, 8, dtype, 1, 'full', 'GPU %s n_j < slab' % dtype, monkeypatch)


@pytest.mark.parametrize('dtype', ['f64', 'bf16'])
def test_workspace_of_a_900_by_700_relation(dtype, monkeypatch):
    """pass_case asserts the workspace below the bound of sparse_dfmf_cases.pass_case plus 64 (n_i + n_j)."""
    FC.pass_case(900, 700, 128, 64, dtype, 2, 'heavy', 'GPU %s 900 x 700' % dtype, monkeypatch)


def test_flag_is_refused_where_it_does_not_apply():
    FC.refused_flag_cases()


@pytest.mark.parametrize('kind', ['missing', 'nan'])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_refused_at_bind(kind, dtype):
    FC.refused_at_bind_case(kind, dtype)


N = {'a': 3000, 'b': 2600, 'c': 500}
RANK_B = {'mean': 64, 'row_mean': 256, 'col_mean': 128, 2.5: 64}


@pytest.mark.parametrize('fill', FC.FILLS)
def test_f64_fit_against_the_oracle_on_the_filled_matrix(fill):
    FC.fit_against_oracle(N, {'a': 128, 'b': RANK_B[fill], 'c': 64}, fill, 'f64', FC.fit_tol('f64'), 'GPU f64 fill %r' % (fill,))


@pytest.mark.parametrize('fill', FC.FILLS)
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_f32_bf16_fit_against_the_f64_oracle(dtype, fill):
    """Against the f64 oracle, not the dense-fed bf16 plan: that plan rounds the fill values to bf16, the list form does not."""
    FC.fit_against_oracle(N, {'a': 128, 'b': RANK_B[fill], 'c': 64}, fill, dtype, FC.fit_tol(dtype),
                          'GPU %s fill %r' % (dtype, fill))


def test_dfmc_row_mean_against_the_dfmc_oracle_and_repeatable():
    ranks = {'a': 128, 'b': 64, 'c': 64}
    FC.fit_against_oracle(N, ranks, 'row_mean', 'f64', FC.fit_tol('f64'), 'GPU DFMC', variant=nat.SKF_DFMC)
    FC.dfmc_repeat_case(N, ranks)
    FC.dfmc_repeat_case(N, ranks, 'bf16')


@pytest.mark.parametrize('fill', FC.FILLS)
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_api_dfmf_never_expands(dtype, fill, monkeypatch):
    """Fails without the feature: Dfmf expands an unstored='unknown' relation to its MaskedArray."""
    FC.api_case(FC.Dfmf, fill, dtype, (900, 700), monkeypatch, ranks=(128, 64, 32), n_g=200)


def test_api_dfmc_line_means_never_expand(monkeypatch):
    for fill in ('row_mean', 'col_mean'):
        FC.api_case(FC.Dfmc, fill, 'f64', (900, 700), monkeypatch, ranks=(128, 64, 32), n_g=200)


def test_api_everything_else(tmp_path, monkeypatch):
    FC.api_everything_else_case((600, 500), 'f64', tmp_path, monkeypatch)
