"""Seed-addressed noise (csrc/philox.h, the Philox kernels of bridge.hip, ``seeds=`` / ``BridgeSampler(noise="philox")``) on the GPU:
the bit stream, the normals against the float64 formula, fused == unfused bit for bit, and the model level against the oracle."""
import pytest
import torch

import philox_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_philox_words_match_the_known_answer_vectors(dev):
    P.bit_stream(dev)


def test_philox_normal_follows_the_formula_and_is_addressed_by_seed_ordinal_domain(dev):
    P.normals(dev)


def test_philox_normal_distribution(dev):
    P.distribution(dev)


@pytest.mark.parametrize("shape,off", [((3, 16, 20), 0), ((3, 321), 1)], ids=["960-aligned", "963-offset4B"])
def test_fused_step_equals_batched_step_fed_the_noise_tensor(dev, shape, off):
    P.fused_step_equals_unfused(dev, shape, off)


@pytest.mark.parametrize("shape,off", [((3, 16, 20), 0), ((3, 321), 1)], ids=["960-aligned", "963-offset4B"])
def test_fused_q_sample_equals_q_sample_fed_the_noise_tensor(dev, shape, off):
    P.fused_q_sample_equals_unfused(dev, shape, off)


def test_philox_sampler_and_model_sample_follow_the_oracle(dev):
    P.model_level(dev)


def test_philox_sampler_issues_no_normal_launch_and_is_reproducible(dev):
    """Default plan (hipGraph on): two samplers over the same seeds give the same bits whatever torch's generator state is, and the
    global generator is not advanced by a philox run."""
    import sampler_cases as S
    from bbdm_amd import BridgeSampler
    m, _ = S.tiny_concat(dev, 6)
    g = torch.Generator().manual_seed(2)
    conds = torch.randn(3, 3, 16, 16, generator=g).clamp(-1, 1).to(dev)
    torch.manual_seed(1)
    state = torch.cuda.get_rng_state(dev)
    s = BridgeSampler(m, 4, noise="philox")
    s.submit([(k, conds[k], 50 + k) for k in range(3)])
    a = dict(s)
    assert torch.equal(torch.cuda.get_rng_state(dev), state)
    torch.manual_seed(99)
    s = BridgeSampler(m, 4, noise="philox")
    s.submit([(k, conds[k], 50 + k) for k in range(3)])
    b = dict(s)
    for k in range(3):
        assert torch.equal(a[k], b[k])


def test_fused_step_with_a_ragged_group_follows_the_formula(dev):
    P.fused_step_follows_the_formula(dev)
