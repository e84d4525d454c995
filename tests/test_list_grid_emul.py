"""Grid, part mapping and error-partial count of the entry-list passes at outer sizes that do not divide evenly, on the host
emulator: every list form at 5 x 33 and 1 x 9, lists in 1 and 8 parts, f64 and f32 at ranks 3 and 8; a 0/1 relation of 69
rows as lists over bf16 rows (tests/list_grid_cases.py)."""
import pytest

from emul.runtime import emulated_runtime, use_runtime

import list_grid_cases as LG


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


FORMS = {'known': LG.known_case, 'stored': LG.stored_case, 'filled': LG.filled_case}


@pytest.mark.parametrize('parts', LG.PARTS)
@pytest.mark.parametrize('rank', [3, 8])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('shape', LG.SHAPES)
@pytest.mark.parametrize('form', sorted(FORMS))
def test_parted_forms_at_uneven_sizes(form, shape, dtype, rank, parts, monkeypatch):
    FORMS[form](shape, rank, dtype, parts, 'emulator %s %d x %d %s rank %d parts %d' % (form, shape[0], shape[1], dtype, rank, parts),
                monkeypatch)


@pytest.mark.parametrize('rank', [3, 8])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('shape', LG.SHAPES)
def test_fold_in_lists_at_uneven_sizes(shape, dtype, rank):
    LG.fold_case(shape, rank, dtype, 'emulator fold-in %d x %d %s rank %d' % (shape[0], shape[1], dtype, rank))


@pytest.mark.parametrize('parts', LG.PARTS)
@pytest.mark.parametrize('ranks', [(64, 128), (128, 64)])
def test_ones_lists_of_69_rows(ranks, parts, monkeypatch):
    for pattern in ('edges', 'heavy'):
        LG.ones_case(ranks, parts, pattern, 'emulator ones 69 rows ranks %d/%d parts %d %s' % (ranks[0], ranks[1], parts, pattern),
                     monkeypatch)
