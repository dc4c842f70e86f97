"""bbdm_amd.optim (fused Adam + EMA) on the CPU-emulated kernels: parity with torch.optim.Adam and with
the reference's EMA class (an inline restatement of its 8 lines: tests/optim_cases.py)."""
import pytest
import torch

import optim_cases as C
from emu_backend import emulated_backend

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


@pytest.mark.parametrize("wd,beta1", [(0.0, 0.9), (0.01, 0.5)])
def test_fused_adam_matches_torch_adam(wd, beta1):
    C.adam_parity(CPU, wd, beta1)


def test_ema_matches_reference_ema_and_fuses_into_the_step():
    C.ema_parity(CPU)


def test_ema_copy_without_adam_leaves_rows_that_carry_gradients_alone():
    C.ema_copy_leaves_gradient_rows_alone(CPU)
