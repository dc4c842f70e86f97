"""Per-request sampling parameters (SamplingParams of bbdm_amd/sampler.py, the two *_requests_* bridge kernels) on the CPU-emulated
kernels (tools/hipemu): the product code paths with every launch executed by the emulator."""
import pytest
import torch

import sampler_params_cases as C
from emu_backend import emulated_backend

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


def test_per_image_eta_and_clip_are_bit_equal_to_the_scalar_step():
    C.kernel_per_image_params(CPU)


@pytest.mark.parametrize("shape,off", [((3, 16, 20), 0), ((3, 16, 20), 1), ((3, 5, 7), 0)], ids=["aligned", "offset4", "ragged"])
def test_per_image_eta_and_clip_philox_are_bit_equal_to_the_scalar_step(shape, off):
    C.kernel_per_image_params_philox(CPU, shape, off)


def test_uniform_params_reproduce_the_batched_entry_points():
    C.kernel_uniform_params(CPU)


def test_requests_entry_points_check_their_arguments():
    C.kernel_argument_checks(CPU)


def test_lockstep_with_uniform_params_equals_the_model_configured_with_them():
    C.lockstep_uniform_params(CPU, hip_graph=False)


@pytest.mark.parametrize("noise", ["torch", "philox"])
def test_mixed_schedules_follow_the_oracle_and_the_slot_simulation(noise):
    C.mixed_schedules(CPU, noise, hip_graph=False)


def test_default_params_equal_the_three_tuple_and_sample_set_takes_params():
    C.defaults_and_sample_set(CPU, hip_graph=False)


def test_params_are_rejected_at_submission():
    C.rejection(CPU)
