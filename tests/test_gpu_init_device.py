"""The column-mean initialisers on the GPU (tests/init_device_cases.py): exact data byte for byte against `_init.initialize`
in every engine, stored form, initialiser and orientation at the shapes that cross a tile, slab or split seam -- relations
67 x 131 / 131 x 40 and 203 x 997 / 997 x 67, ranks (5, 7), (64, 65) and (128, 200), 600 rows for several norm slabs --,
the pools of `random_c`, the line norms, real-valued data under the derived bound, every refusal under guard bands, the
public API."""
import pytest

import init_device_cases as IC

pytestmark = pytest.mark.gpu

SMALL, BIG = (67, 131, 40), (203, 997, 67)


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
@pytest.mark.parametrize('form', ['dense', 'csr'])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_exact_byte_for_byte(dtype, form, init_type):
    IC.exact_case(dtype, SMALL, (5, 7, 5), 'ratings', form, init_type)
    IC.exact_case(dtype, BIG, (64, 65, 64), 'ratings', form, init_type)


@pytest.mark.parametrize('form', ['dense', 'csr'])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_exact_rank_above_a_tile(dtype, form):
    IC.exact_case(dtype, BIG, (128, 200, 128), 'ratings', form, 'random_c')
    IC.exact_case(dtype, (600, 131, 300), (128, 200, 128), 'ratings', form, 'random_vcol')


@pytest.mark.parametrize('kind', ['binary', 'ones'])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_exact_zero_one_relations(dtype, kind):
    """SKF_BF16 keeps these as bitmaps (the sparse one as lists of its ones beside it); columns tie heavily."""
    IC.exact_case(dtype, SMALL, (5, 7, 5), kind, 'dense', 'random_c')
    IC.exact_case(dtype, BIG, (64, 65, 64), kind, 'dense', 'random_c')
    IC.exact_case(dtype, BIG, (128, 200, 128), kind, 'dense', 'random_vcol')


@pytest.mark.parametrize('dtype,kind,form', [('f64', 'ratings', 'dense'), ('f32', 'ratings', 'dense'), ('f32', 'ratings', 'csr'),
                                             ('f64', 'ratings', 'csr'), ('bf16', 'ratings', 'dense'), ('bf16', 'binary', 'dense'),
                                             ('bf16', 'ratings', 'csr')])
def test_norms_exact_over_several_slabs(dtype, kind, form):
    IC.norms_case(dtype, (600, 131, 300), kind, form)
    IC.norms_case(dtype, BIG, kind, form)


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
@pytest.mark.parametrize('ranks', [(5, 7, 5), (64, 65, 64), (128, 200, 128)])
@pytest.mark.parametrize('dtype,form', [('f64', 'dense'), ('f32', 'dense'), ('f64', 'csr'), ('f32', 'csr')])
def test_real_data_under_the_derived_bound(dtype, form, ranks, init_type):
    IC.real_case(dtype, SMALL, ranks, form, init_type)
    IC.real_case(dtype, BIG, ranks, form, init_type)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_refusals_and_guards(dtype):
    IC.refusals_case(dtype)


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
@pytest.mark.parametrize('kind', ['dense', 'sparse', 'binary'])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
@pytest.mark.parametrize('cls', ['Dfmf', 'Dfmc'])
def test_public_api_equals_the_host_initialiser(cls, dtype, kind, init_type, monkeypatch):
    IC.api_case(cls, dtype, kind, init_type, monkeypatch)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
@pytest.mark.parametrize('cls', ['Dfmf', 'Dfmc'])
def test_public_api_restarts(cls, dtype, monkeypatch):
    """n_run = 3 with n_jobs = 2: shared launches of a small graph (Dfmf, f64 / f32) / restarts side by side on streams."""
    IC.api_case(cls, dtype, 'dense', 'random_c', monkeypatch, n_run=3, n_jobs=2)


@pytest.mark.parametrize('cls,what', [('Dfmc', 'masked'), ('Dfmf', 'narrow'), ('Dfmf', 'random'), ('Dfmc', 'random')])
def test_ineligible_fits_stay_on_the_host(cls, what):
    IC.ineligible_case(cls, what)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_device_fill_with_the_default_initialiser(dtype, monkeypatch):
    IC.device_fill_case(dtype, monkeypatch)
