"""The column-mean initialisers for relations with missing values on the GPU (tests/init_known_cases.py): exact data byte for
byte against `_init.initialize` in every engine, initialiser and list form -- relations 67 x 131 / 131 x 40 and 203 x 997 /
997 x 67, ranks (5, 7), (64, 65) and (128, 200): one, two and four factor columns per lane, ranks that are no multiple of
64 --, hand-made selections and the mixed type in both view orders, a relation without entries, the line norms over several
hundred lines, mask-fed against CSR-fed lists, real-valued data under the derived bound, every refusal under guard bands, the
public API."""
import pytest

import init_known_cases as KC

pytestmark = pytest.mark.gpu

SMALL, BIG = (67, 131, 40), (203, 997, 67)
FORMS = [('known', 2.5), ('rank1', 2.5), ('rank1', 'mean'), ('rank1', 'row_mean'), ('rank1', 'col_mean')]


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
@pytest.mark.parametrize('form,fill', FORMS)
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_exact_byte_for_byte(dtype, form, fill, init_type):
    KC.exact_case(dtype, SMALL, (5, 7, 5), form, fill, init_type)
    KC.exact_case(dtype, BIG, (64, 65, 64), form, fill, init_type)


@pytest.mark.parametrize('form,fill', FORMS)
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_exact_rank_above_a_lane_block(dtype, form, fill):
    KC.exact_case(dtype, BIG, (128, 200, 128), form, fill, 'random_c')
    KC.exact_case(dtype, (600, 131, 300), (128, 200, 128), form, fill, 'random_vcol')


@pytest.mark.parametrize('form,fill', [('known', 2.5), ('rank1', 2.5), ('rank1', 'mean')])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_exact_empty_and_full_columns(dtype, form, fill):
    """The pattern transposed: the empty and the full line are columns of the relation."""
    KC.exact_case(dtype, SMALL, (5, 7, 5), form, fill, 'random_c', flip=True)
    KC.exact_case(dtype, BIG, (64, 65, 64), form, fill, 'random_vcol', flip=True)


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_no_stored_entry_at_all(dtype, init_type):
    KC.exact_case(dtype, SMALL, (5, 7, 5), 'known', 2.5, init_type, empty=True)


@pytest.mark.parametrize('form,fill', FORMS)
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_chosen_by_all_chosen_by_none_and_both_view_orders(dtype, form, fill):
    KC.chosen_columns_case(dtype, form, fill)
    KC.chosen_columns_case(dtype, form, fill, BIG, (64, 65, 64))


@pytest.mark.parametrize('form,fill,flip', [('known', 2.5, False), ('known', 2.5, True), ('rank1', 2.5, False), ('rank1', 'mean', False),
                                            ('rank1', 'mean', True), ('rank1', 'row_mean', False), ('rank1', 'col_mean', False)])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_line_norms_exact(dtype, form, fill, flip):
    KC.norms_case(dtype, (600, 131, 300), form, fill, flip)
    KC.norms_case(dtype, BIG, form, fill, flip)


@pytest.mark.parametrize('form', ['dense', 'csr'])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_older_forms_take_the_unchanged_route(dtype, form):
    KC.unchanged_route_case(dtype, form)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_mask_fed_equals_csr_fed(dtype):
    KC.mask_fed_case(dtype)


@pytest.mark.parametrize('ranks', [(5, 7, 5), (64, 65, 64), (128, 200, 128)])
@pytest.mark.parametrize('form,fill', [('known', 'mean'), ('rank1', 'mean'), ('rank1', 'row_mean')])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_real_data_under_the_derived_bound(dtype, form, fill, ranks):
    KC.real_case(dtype, SMALL, ranks, form, fill)
    KC.real_case(dtype, BIG, ranks, form, fill)


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_refusals_and_guards(dtype):
    KC.refusals_case(dtype)


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
@pytest.mark.parametrize('fill', [2.5, 'row_mean'])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
@pytest.mark.parametrize('cls', ['Dfmf', 'Dfmc'])
def test_public_api_equals_the_host_initialiser(cls, dtype, fill, init_type, monkeypatch):
    KC.api_case(cls, dtype, fill, init_type, monkeypatch)


@pytest.mark.parametrize('cls', ['Dfmf', 'Dfmc'])
def test_public_api_restarts(cls, monkeypatch):
    """n_run = 3 with n_jobs = 2: restarts side by side on streams, one shared upload of the lists."""
    KC.api_case(cls, 'f32', 2.5, 'random_c', monkeypatch, n_run=3, n_jobs=2)
