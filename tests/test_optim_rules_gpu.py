"""FusedSGD / FusedRMSprop of bbdm_amd.optim on the GPU (bodies: tests/optim_rules_cases.py), against torch's optimizers on a CPU copy."""
import pytest
import torch

import optim_rules_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("momentum,dampening,nesterov,wd", C.SGD_GRID)
def test_fused_sgd_matches_torch_sgd(dev, momentum, dampening, nesterov, wd):
    C.sgd_parity(dev, momentum, dampening, nesterov, wd)


@pytest.mark.parametrize("momentum,wd,alpha", C.RMSPROP_GRID)
def test_fused_rmsprop_matches_torch_rmsprop(dev, momentum, wd, alpha):
    C.rmsprop_parity(dev, momentum, wd, alpha)


def test_sgd_first_step_with_dampening_copies_the_gradient(dev):
    C.sgd_first_step_with_dampening(dev)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("rule", C.RULES)
def test_ragged_and_unaligned_chunks(dev, rule, clip):
    C.ragged(dev, rule, clip)


@pytest.mark.parametrize("rule", C.RULES)
def test_fused_ema_matches_step_then_update_and_the_reference_ema(dev, rule):
    C.fused_ema(dev, rule)


@pytest.mark.parametrize("max_norm", [0.5, 1e9])
@pytest.mark.parametrize("rule", C.RULES)
def test_clipping_inside_the_pass(dev, rule, max_norm):
    C.clipping(dev, rule, max_norm)


@pytest.mark.parametrize("rule", C.RULES)
def test_guard_skips_the_step(dev, rule):
    C.guard(dev, rule)


@pytest.mark.parametrize("rule", C.RULES)
def test_without_guard_nonfinite_propagates(dev, rule):
    C.no_guard_propagates(dev, rule)


def test_sgd_skipped_first_step_leaves_a_zero_buffer(dev):
    C.sgd_skipped_first_step(dev)


@pytest.mark.parametrize("rule", C.RULES)
def test_clipped_steps_are_reproducible(dev, rule):
    C.reproducible(dev, rule)


@pytest.mark.parametrize("rule", C.RULES)
def test_state_dict_round_trips_with_torch(dev, rule):
    C.state_dict_round_trip(dev, rule)


def test_centered_rmsprop_is_refused(dev):
    C.centered_is_refused(dev)


@pytest.mark.parametrize("rule", C.RULES)
def test_reduce_lr_on_plateau(dev, rule):
    C.plateau_scheduler(dev, rule)


def test_get_optimizer_returns_the_fused_classes(dev):
    C.get_optimizer_cases(dev)


def test_cpu_parameters_are_refused(dev):
    C.cpu_parameters_are_refused()
