"""Gradient-norm clipping and the non-finite guard of bbdm_amd.optim on the CPU-emulated kernels (bodies: tests/optim_clip_cases.py)."""
import pytest
import torch

import optim_clip_cases as C
from emu_backend import emulated_backend

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_clipped_fused_adam_matches_torch_clip_and_adam(wd):
    C.parity(CPU, wd)


def test_clip_grad_norm_matches_torch_and_step_override():
    C.standalone_clip_parity(CPU)


def test_norm_accuracy_against_fp64():
    C.norm_accuracy(CPU)


def test_norm_window():
    C.norm_window(CPU)


def test_norm_is_order_independent():
    C.order_independence(CPU)


def test_loose_bound_is_bitwise_identity():
    C.loose_bound_is_identity(CPU)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_guard_skips_the_step(bad):
    C.guard(CPU, bad)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_without_guard_nonfinite_propagates(bad):
    C.no_guard_propagates(CPU, bad)


def test_interface():
    C.interface(CPU)
