"""Evaluation metrics (bbdm_amd/metrics.py, csrc/metrics.hip) on the GPU: the cases of tests/metrics_cases.py, plus a batch against
the same images one at a time and the evaluator fed by a BridgeSampler run."""
import pytest
import torch

import metrics_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("shape", C.SHAPES)
def test_pair_sums_are_the_exact_integers(dev, shape):
    C.pair_sums_exact(dev, shape)


@pytest.mark.parametrize("kind", ["random", "flat", "pm2", "same"])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_ssim_matches_the_float64_2d_convolution(dev, shape, kind):
    C.ssim_matches(dev, shape, kind)


def test_ssim_rejects_images_smaller_than_the_window(dev):
    C.ssim_rejects_small(dev)


@pytest.mark.parametrize("shape", C.DIVERSITY_SHAPES)
def test_diversity_matches_the_reference_fp32_formula(dev, shape):
    C.diversity_matches(dev, shape)


def test_diversity_of_identical_samples_is_exactly_zero(dev):
    C.diversity_of_identical_samples_is_zero(dev)


def test_float_input_is_quantised_like_the_png_writer(dev):
    C.float_input_is_quantised_like_the_png_writer(dev)


def test_raw_cells_are_bitwise_repeatable_and_batch_independent(dev):
    C.raw_cells_repeat(dev, one_at_a_time=True)


def test_metrics_from_files_equal_metrics_from_tensors(dev, tmp_path):
    C.files_equal_tensors(dev, tmp_path)


def test_set_evaluator_in_any_arrival_order(dev):
    C.evaluator_in_any_arrival_order(dev)


def test_set_evaluator_consumes_a_bridge_sampler(dev):
    C.evaluator_consumes_a_sampler(dev)
