"""scipy.sparse relations (unstored entries zero) through Dfmf / Dfmc on the host emulator: the eligible ones are fitted on
their stored entries and never expanded, every other case reproduces the toarray() fit bit for bit, the initialisers read
their statistics from the entries (tests/sparse_dfmf_api_cases.py)."""
import pytest

from emul.runtime import emulated_runtime, use_runtime
from skfusion_amd.fusion import Dfmf, Dfmc

import sparse_dfmf_api_cases as AC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


N = (60, 50)


@pytest.mark.parametrize('cls', [Dfmf, Dfmc])
@pytest.mark.parametrize('dtype', ['f64', 'f32', 'bf16'])
def test_eligible_relation_is_never_expanded(cls, dtype, monkeypatch):
    AC.eligible_case(cls, dtype, N, monkeypatch, sparse_relations=True)


def test_eligible_relation_on_the_pipeline_schedule(monkeypatch):
    AC.eligible_case(Dfmf, 'f64', (300, 260), monkeypatch, ranks=(70, 66, 68), n_g=150, init_type='random')                    # (the default rule takes it)


@pytest.mark.parametrize('cls', [Dfmf, Dfmc])
def test_ineligible_relations_expand_as_before(cls):
    AC.ineligible_cases(cls, 'f64', N)


@pytest.mark.parametrize('init_type', ['random_c', 'random_vcol'])
def test_initialisers_read_the_entries(init_type):
    AC.initialiser_case(N, init_type)


def test_stopping_and_errors_through_the_error_pass():
    AC.stopping_case(N)


def test_concurrent_restarts_share_the_lists(monkeypatch):
    AC.restarts_case(N, 'f64', monkeypatch)


def test_complete_save_load(tmp_path):
    AC.complete_save_load_case(N, 'f64', tmp_path)
