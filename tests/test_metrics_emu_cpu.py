"""Evaluation metrics (bbdm_amd/metrics.py, csrc/metrics.hip) on the CPU-emulated kernels: exact pair sums, fp64 SSIM against a
2-D float64 convolution, the reference's fp32 diversity, bitwise repeatability, files == tensors, the streaming evaluator."""
import pytest
import torch

import metrics_cases as C
from emu_backend import emulated_backend

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


@pytest.mark.parametrize("shape", C.SHAPES)
def test_pair_sums_are_the_exact_integers(shape):
    C.pair_sums_exact(CPU, shape)


@pytest.mark.parametrize("kind", ["random", "flat", "pm2", "same"])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_ssim_matches_the_float64_2d_convolution(shape, kind):
    C.ssim_matches(CPU, shape, kind)


def test_ssim_rejects_images_smaller_than_the_window():
    C.ssim_rejects_small(CPU)


@pytest.mark.parametrize("shape", C.DIVERSITY_SHAPES)
def test_diversity_matches_the_reference_fp32_formula(shape):
    C.diversity_matches(CPU, shape)


def test_diversity_of_identical_samples_is_exactly_zero():
    C.diversity_of_identical_samples_is_zero(CPU)


def test_float_input_is_quantised_like_the_png_writer():
    C.float_input_is_quantised_like_the_png_writer(CPU)


def test_raw_cells_are_bitwise_repeatable():
    C.raw_cells_repeat(CPU, one_at_a_time=True)


def test_metrics_from_files_equal_metrics_from_tensors(tmp_path):
    C.files_equal_tensors(CPU, tmp_path)


def test_set_evaluator_in_any_arrival_order():
    C.evaluator_in_any_arrival_order(CPU)
