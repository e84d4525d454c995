"""Held-out pairs scored inside the fit (csrc/skf_heldout.h, skf_plan_set_heldout, DevicePlan.set_heldout, Dfmf / Dfmc
``validation=``) on the MI355X: the operator bit for bit against host arithmetic in the kernel's documented order and against
a pure-f64 model within its derived bound at every width class and at c_j = 1023 (the widest rank a plan takes), every refusal, fits that monitoring does
not perturb, the history, the best iterate, the patience mechanics and the API surface (tests/heldout_cases.py)."""
import pytest

import heldout_cases as HC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('cj', [1, 5, 16, 17, 63, 64, 65, 130])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_operator_against_host_arithmetic(dtype, cj):
    HC.operator_case(dtype, 37, 41, 5 if cj != 5 else 17, cj, HC.sizes_for(cj), 'GPU')


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_operator_widest(dtype):
    """The widest column type a plan can have: skf_plan_create takes ranks up to 1023 (the order limit of its
    pseudo-inverse), so c_j = 1024 -- the limit of the entry kernels -- cannot be reached through a plan; 9 rows."""
    HC.operator_case(dtype, 9, 41, 20, 1023, [(1025, 'corner'), (3, 'one_row')], 'GPU')


@pytest.mark.parametrize('ci,cj', [(64, 128), (128, 64)])
def test_operator_bf16_plan_scores_on_its_f32_masters(ci, cj):
    HC.operator_case('bf16', 37, 41, ci, cj, [(1025, 'dups'), (2500, 'corner')], 'GPU')


def test_refusals_at_the_c_abi():
    HC.refusals_case()


@pytest.mark.parametrize('ranks,forced', [(HC.RANKS_SMALL, False), (HC.RANKS_WIDE, True)])
def test_monitoring_does_not_perturb_the_fit(ranks, forced, monkeypatch):
    HC.no_perturbation_case(ranks, forced, monkeypatch)


@pytest.mark.parametrize('ranks', [HC.RANKS_SMALL, HC.RANKS_WIDE])
def test_history_is_the_truth(ranks):
    HC.history_case(ranks)


def test_best_iterate_is_kept_and_returned():
    HC.best_iterate_case()


def test_patience_mechanics():
    HC.patience_case(HC.RANKS_SMALL)


def test_callback_and_error_logging_alongside():
    HC.alongside_case(HC.RANKS_SMALL)


def test_nan_total_never_improves():
    HC.nan_case()


@pytest.mark.parametrize('cls', ['Dfmc', 'Dfmf'])
def test_api_heldout_formats(cls):
    HC.api_formats_case(cls)


def test_api_two_lists_restarts_and_plain_fit():
    HC.api_two_lists_and_runs_case()


def test_api_dfmf_early_stop_returns_best():
    HC.api_dfmf_case()


def test_api_refusals():
    HC.api_refusals_case()
