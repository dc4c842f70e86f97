"""The tiny-UNet tests of test_wide_heads_model_gpu.py (128-channel attention heads: AttentionBlock in both head orders and a
SpatialTransformer with a context; sampling forward and loss + all parameter gradients against the oracle, bitwise reproducible training
step) on the CPU-emulated kernels (tools/hipemu)."""
import pytest
import torch

import test_fullsize_parity_gpu as FS
import test_wide_heads_model_gpu as WM
from emu_backend import emulated_backend

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


@pytest.fixture(autouse=True)
def eager_plans(monkeypatch):
    """No hipGraph on the emulator: the plans run launch by launch."""
    real = FS._model

    def build(up, bb, seed, dev):
        m, sd = real(up, bb, seed, dev)
        m.denoise_fn.hip_graph = False
        return m, sd
    monkeypatch.setattr(FS, "_model", build)


@pytest.mark.parametrize("variant", list(WM.VARIANTS))
def test_tiny_unet_forward_matches_oracle(variant):
    WM.test_tiny_unet_forward_matches_oracle(CPU, variant)


@pytest.mark.parametrize("variant", list(WM.VARIANTS))
def test_tiny_unet_loss_and_all_gradients(variant):
    WM.test_tiny_unet_loss_and_all_gradients(CPU, variant)
