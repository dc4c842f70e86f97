"""Per-request sampling parameters (SamplingParams of bbdm_amd/sampler.py, the two *_requests_* bridge kernels) on the GPU."""
import pytest
import torch

import sampler_params_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_per_image_eta_and_clip_are_bit_equal_to_the_scalar_step(dev):
    C.kernel_per_image_params(dev)


@pytest.mark.parametrize("shape,off", [((3, 16, 20), 0), ((3, 16, 20), 1), ((3, 5, 7), 0)], ids=["aligned", "offset4", "ragged"])
def test_per_image_eta_and_clip_philox_are_bit_equal_to_the_scalar_step(dev, shape, off):
    C.kernel_per_image_params_philox(dev, shape, off)


def test_uniform_params_reproduce_the_batched_entry_points(dev):
    C.kernel_uniform_params(dev)


def test_requests_entry_points_check_their_arguments(dev):
    C.kernel_argument_checks(dev)


def test_lockstep_with_uniform_params_equals_the_model_configured_with_them(dev):
    C.lockstep_uniform_params(dev)


@pytest.mark.parametrize("noise", ["torch", "philox"])
def test_mixed_schedules_follow_the_oracle_and_the_slot_simulation(dev, noise):
    C.mixed_schedules(dev, noise)


def test_default_params_equal_the_three_tuple_and_sample_set_takes_params(dev):
    C.defaults_and_sample_set(dev)


def test_params_are_rejected_at_submission(dev):
    C.rejection(dev)
