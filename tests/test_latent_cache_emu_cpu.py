"""Latent cache (the cached q_sample kernels and the channel statistics of csrc/bridge.hip, bbdm_amd/latent_cache.py, the index path
of LatentBrownianBridgeModel.forward) on the CPU-emulated kernels (tools/hipemu): the product code paths with every launch executed
by the emulator.  The out-of-range cases live here only, so that they also run under the emulator's sanitizer build."""
import pytest
import torch

import latent_cache_cases as L
from emu_backend import emulated_backend

CPU = torch.device("cpu")
SHAPES = pytest.mark.parametrize("shape,off", [((3, 16, 20), 0), ((3, 321), 1)], ids=["960-aligned", "963-offset4B"])
NOISE = pytest.mark.parametrize("philox", [False, True], ids=["tensor", "philox"])


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


@SHAPES
@NOISE
def test_cached_q_sample_equals_q_sample_fed_the_gathered_rows(shape, off, philox):
    L.kernel_equals_unfused(CPU, shape, off, philox)


@SHAPES
@NOISE
def test_out_of_range_index_gives_nan_rows_and_touches_no_other_image(shape, off, philox):
    L.out_of_range_rows_are_nan(CPU, shape, off, philox)


def test_index_inputs_are_checked_on_the_host():
    L.index_input_errors(CPU)


def test_channel_stats_are_exact_and_order_independent():
    L.channel_stats(CPU, nan_row=True)


def test_cache_equals_encode_and_round_trips(tmp_path):
    L.cache_equals_encode(CPU, tmp_path)


@pytest.mark.parametrize("seeded", [False, True], ids=["torch-noise", "seeds"])
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
def test_training_step_on_indices_equals_the_step_on_images(monkeypatch, normalize, loss_type, seeded):
    L.training_step_index_equals_image(CPU, monkeypatch, normalize, loss_type, seeded)


def test_float_inputs_keep_their_path_after_attach():
    L.float_inputs_keep_their_path(CPU)


def test_cached_pairs_feed_the_runner_loss_fn():
    L.runner_seam(CPU)


@NOISE
def test_cached_q_sample_with_a_ragged_group_follows_the_formula(philox):
    L.ragged_group_follows_the_formula(CPU, philox)
