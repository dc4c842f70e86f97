"""BridgeSampler (bbdm_amd/sampler.py) and its per-image bridge kernel on the CPU-emulated kernels (tools/hipemu): the product code
paths with every launch executed by the emulator."""
import pytest
import torch

import sampler_cases as S
from emu_backend import emulated_backend

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


def test_batched_bridge_step_is_bit_equal_to_the_scalar_step():
    S.kernel_equivalence(CPU)


def test_sampler_with_refills_and_idle_tail_follows_the_oracle():
    """tiny_concat's UNet, sample_step 6, width 3, 5 requests arriving in three groups: refills mid-flight and an idle tail; each
    request within 5e-3 of its own oracle loop, every key once; then sample_set's shape (and values) on the same sampler."""
    m, s, conds, seeds, ora = S.mixed_progress(CPU, 3, 5, 6, clip=True, hip_graph=False)
    S.sample_set_shape(CPU, s, conds, seeds, ora, clip=True)


def test_sampler_rejects_at_submission():
    S.rejection(CPU)
