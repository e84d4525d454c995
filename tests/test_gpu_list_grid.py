"""Grid, part mapping and error-partial count of the entry-list passes at outer sizes that do not divide evenly, on the
MI355X: every list form at 5 x 33 and 1 x 9, lists in 1 and 8 parts, f64 at rank 8 and bf16 at rank 128 (the row type's:
srp_bf16_v6_kernel for the known-entry passes and Q of the stored entries, srp_bf16_kernel for the error pass of the known
entries; the column type's rank is 3, list_grid_cases.ranks_of); a 0/1 relation of 69 rows as lists over bf16 rows
(tests/list_grid_cases.py)."""
import pytest

import list_grid_cases as LG

pytestmark = pytest.mark.gpu

ENGINES = [('f64', 8), ('bf16', 128)]
FORMS = {'known': LG.known_case, 'stored': LG.stored_case, 'filled': LG.filled_case}


@pytest.mark.parametrize('parts', LG.PARTS)
@pytest.mark.parametrize('dtype,rank', ENGINES)
@pytest.mark.parametrize('shape', LG.SHAPES)
@pytest.mark.parametrize('form', sorted(FORMS))
def test_parted_forms_at_uneven_sizes(form, shape, dtype, rank, parts, monkeypatch):
    FORMS[form](shape, rank, dtype, parts, 'GPU %s %d x %d %s rank %d parts %d' % (form, shape[0], shape[1], dtype, rank, parts),
                monkeypatch)


@pytest.mark.parametrize('dtype,rank', ENGINES)
@pytest.mark.parametrize('shape', LG.SHAPES)
def test_fold_in_lists_at_uneven_sizes(shape, dtype, rank):
    LG.fold_case(shape, rank, dtype, 'GPU fold-in %d x %d %s rank %d' % (shape[0], shape[1], dtype, rank))


@pytest.mark.parametrize('parts', LG.PARTS)
@pytest.mark.parametrize('ranks', [(64, 128), (128, 64)])
def test_ones_lists_of_69_rows(ranks, parts, monkeypatch):
    for pattern in ('edges', 'heavy'):
        LG.ones_case(ranks, parts, pattern, 'GPU ones 69 rows ranks %d/%d parts %d %s' % (ranks[0], ranks[1], parts, pattern),
                     monkeypatch)
