"""Seed-addressed noise (csrc/philox.h, the Philox kernels of bridge.hip, ``seeds=`` / ``BridgeSampler(noise="philox")``) on the
CPU-emulated kernels (tools/hipemu): the product code paths with every launch executed by the emulator."""
import pytest
import torch

import philox_cases as P
from emu_backend import emulated_backend

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


def test_philox_words_match_the_known_answer_vectors():
    P.bit_stream(CPU)


def test_philox_normal_follows_the_formula_and_is_addressed_by_seed_ordinal_domain():
    P.normals(CPU)


def test_philox_normal_distribution():
    P.distribution(CPU)


@pytest.mark.parametrize("shape,off", [((3, 16, 20), 0), ((3, 321), 1)], ids=["960-aligned", "963-offset4B"])
def test_fused_step_equals_batched_step_fed_the_noise_tensor(shape, off):
    P.fused_step_equals_unfused(CPU, shape, off)


@pytest.mark.parametrize("shape,off", [((3, 16, 20), 0), ((3, 321), 1)], ids=["960-aligned", "963-offset4B"])
def test_fused_q_sample_equals_q_sample_fed_the_noise_tensor(shape, off):
    P.fused_q_sample_equals_unfused(CPU, shape, off)


def test_philox_sampler_and_model_sample_follow_the_oracle():
    P.model_level(CPU, hip_graph=False, extras=False)


def test_fused_step_with_a_ragged_group_follows_the_formula():
    P.fused_step_follows_the_formula(CPU)
