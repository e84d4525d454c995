"""The fold-in (SKF_TRANSFORM) on the hardware, stage by stage against the host model of tests/foldin_cases.py (the error
model behind every bound is its module comment): the contractions against the frozen partner factors, every iteration
from the device's previous factor on the fused path (all three foldin_step_kernel instantiations) and on the generic
path (dense and CSR constraints in every engine, the VALU engine in f32 and f64), iterate(k) against k single
iterations, the re-preparation after set_backbone / set_factor, relation_sqerr; object counts 1 .. 4099, target ranks
1 .. 320.  Batches of 1, 2, 16, 17, 33 and 64 plans: each plan the bits of the plan alone, held to its own model; 65
plans and a plan with a target constraint refused."""
import pytest

import foldin_cases as FC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', sorted(FC.GPU))
def test_fold_in_against_host_model(case):
    FC.fold_case(*FC.GPU[case], what='GPU fold-in ' + case)


@pytest.mark.parametrize('case', sorted(FC.BATCH))
def test_batched_fold_ins_against_host_model(case):
    FC.batch_case(*FC.BATCH[case], what='GPU fold-in ' + case)
