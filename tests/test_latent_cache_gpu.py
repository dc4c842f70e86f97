"""Latent cache (the cached q_sample kernels and the channel statistics of csrc/bridge.hip, bbdm_amd/latent_cache.py, the index path
of LatentBrownianBridgeModel.forward) on the GPU: fused == unfused bit for bit, the statistics against float64, the cache against
encode, and the training step on indices against the step on images."""
import pytest
import torch

import latent_cache_cases as L

pytestmark = pytest.mark.gpu
SHAPES = pytest.mark.parametrize("shape,off", [((3, 16, 20), 0), ((3, 321), 1)], ids=["960-aligned", "963-offset4B"])
NOISE = pytest.mark.parametrize("philox", [False, True], ids=["tensor", "philox"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@SHAPES
@NOISE
def test_cached_q_sample_equals_q_sample_fed_the_gathered_rows(dev, shape, off, philox):
    L.kernel_equals_unfused(dev, shape, off, philox)


def test_channel_stats_are_exact_and_order_independent(dev):
    L.channel_stats(dev)


def test_cache_equals_encode_and_round_trips(dev, tmp_path):
    L.cache_equals_encode(dev, tmp_path)


@pytest.mark.parametrize("seeded", [False, True], ids=["torch-noise", "seeds"])
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
def test_training_step_on_indices_equals_the_step_on_images(dev, monkeypatch, normalize, loss_type, seeded):
    L.training_step_index_equals_image(dev, monkeypatch, normalize, loss_type, seeded)


def test_float_inputs_keep_their_path_after_attach(dev):
    L.float_inputs_keep_their_path(dev)


@NOISE
def test_cached_q_sample_with_a_ragged_group_follows_the_formula(dev, philox):
    L.ragged_group_follows_the_formula(dev, philox)
