"""Relations with missing values as entries plus rank one, the host side (no engine): Relation.filled_entries() against
Relation.filled() of the MaskedArray form, what filled_entries_apply takes and leaves, and the initialisers on the entries
view against the expanded filled matrix."""
import pytest

import filled_entries_cases as FC


@pytest.fixture(scope='module', autouse=True)
def no_clamps():
    """No engine runs here: the emulated library's counter of clamped split-K launches stays where it was."""
    from emul.runtime import emulated_runtime
    from skfusion_amd._engine import split_clamps
    rt = emulated_runtime()
    before = split_clamps(rt)
    yield
    assert split_clamps(rt) - before == 0


@pytest.mark.parametrize('fill', FC.FILLS)
def test_container_expands_to_the_filled_masked_array(fill):
    FC.container_case(fill)


def test_what_is_taken_and_what_is_expanded():
    """A stored NaN, every entry stored, a preprocessor, shard='owned' (and the other shard modes): expanded as before."""
    from emul.runtime import emulated_runtime, use_runtime
    with use_runtime(emulated_runtime()):           # (the default rule asks the library for its small-graph limits)
        FC.routing_case()


@pytest.mark.parametrize('fill', FC.FILLS)
@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
def test_initialisers_on_the_entries_view(init_type, fill):
    FC.initialiser_case(init_type, fill)
