"""FusedSGD / FusedRMSprop of bbdm_amd.optim on the CPU-emulated kernels (bodies: tests/optim_rules_cases.py)."""
import pytest
import torch

import optim_rules_cases as C
from emu_backend import emulated_backend

CPU = torch.device("cpu")


@pytest.fixture
def emu():
    """Per test, not per module: the last test of this file needs the REAL library's refusal of CPU tensors."""
    with emulated_backend() as e:
        yield e


@pytest.mark.parametrize("momentum,dampening,nesterov,wd", C.SGD_GRID)
def test_fused_sgd_matches_torch_sgd(emu, momentum, dampening, nesterov, wd):
    C.sgd_parity(CPU, momentum, dampening, nesterov, wd)


@pytest.mark.parametrize("momentum,wd,alpha", C.RMSPROP_GRID)
def test_fused_rmsprop_matches_torch_rmsprop(emu, momentum, wd, alpha):
    C.rmsprop_parity(CPU, momentum, wd, alpha)


def test_sgd_first_step_with_dampening_copies_the_gradient(emu):
    C.sgd_first_step_with_dampening(CPU)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("rule", C.RULES)
def test_ragged_and_unaligned_chunks(emu, rule, clip):
    C.ragged(CPU, rule, clip)


@pytest.mark.parametrize("rule", C.RULES)
def test_fused_ema_matches_step_then_update_and_the_reference_ema(emu, rule):
    C.fused_ema(CPU, rule)


@pytest.mark.parametrize("max_norm", [0.5, 1e9])
@pytest.mark.parametrize("rule", C.RULES)
def test_clipping_inside_the_pass(emu, rule, max_norm):
    C.clipping(CPU, rule, max_norm)


@pytest.mark.parametrize("rule", C.RULES)
def test_guard_skips_the_step(emu, rule):
    C.guard(CPU, rule)


@pytest.mark.parametrize("rule", C.RULES)
def test_without_guard_nonfinite_propagates(emu, rule):
    C.no_guard_propagates(CPU, rule)


def test_sgd_skipped_first_step_leaves_a_zero_buffer(emu):
    C.sgd_skipped_first_step(CPU)


@pytest.mark.parametrize("rule", C.RULES)
def test_clipped_steps_are_reproducible(emu, rule):
    C.reproducible(CPU, rule)


@pytest.mark.parametrize("rule", C.RULES)
def test_state_dict_round_trips_with_torch(emu, rule):
    C.state_dict_round_trip(CPU, rule)


def test_centered_rmsprop_is_refused(emu):
    C.centered_is_refused(CPU)


@pytest.mark.parametrize("rule", C.RULES)
def test_reduce_lr_on_plateau(emu, rule):
    C.plateau_scheduler(CPU, rule)


def test_get_optimizer_returns_the_fused_classes(emu):
    C.get_optimizer_cases(CPU)


def test_cpu_parameters_are_refused_without_the_emulator():
    C.cpu_parameters_are_refused()
