"""Held-out pairs scored inside the fit (csrc/skf_heldout.h, skf_plan_set_heldout, DevicePlan.set_heldout, Dfmf / Dfmc
``validation=``) on the host emulator: the operator bit for bit against host arithmetic in the kernel's documented order and
against a pure-f64 model within its derived bound, every refusal, fits that monitoring does not perturb, the history, the
best iterate, the patience mechanics and the API surface (tests/heldout_cases.py)."""
import pytest

from emul.runtime import emulated_runtime, use_runtime

import heldout_cases as HC


@pytest.fixture(scope='module', autouse=True)
def emul():
    from skfusion_amd._engine import split_clamps
    with use_runtime(emulated_runtime()) as rt:
        yield rt
        assert split_clamps(rt) == 0


@pytest.mark.parametrize('cj', [1, 5, 16, 17, 63, 64, 65, 130])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_operator_against_host_arithmetic(dtype, cj):
    HC.operator_case(dtype, 37, 41, 5 if cj != 5 else 17, cj, HC.sizes_for(cj), 'emulator')


@pytest.mark.parametrize('ci,cj', [(64, 128), (128, 64)])
def test_operator_bf16_plan_scores_on_its_f32_masters(ci, cj):
    HC.operator_case('bf16', 37, 41, ci, cj, [(1025, 'dups'), (2500, 'corner')], 'emulator')


def test_refusals_at_the_c_abi():
    HC.refusals_case()


@pytest.mark.parametrize('ranks,forced', [(HC.RANKS_SMALL, False), (HC.RANKS_WIDE, True)])
def test_monitoring_does_not_perturb_the_fit(ranks, forced, monkeypatch):
    HC.no_perturbation_case(ranks, forced, monkeypatch)


def test_history_is_the_truth():
    HC.history_case(HC.RANKS_SMALL)


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
