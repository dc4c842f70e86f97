"""Weight packing (bbdm_amd/packing.py) on the CPU-emulated kernels (tools/hipemu): the one refresh protocol over every packer and
plane layout the planner can construct, bit for bit."""
import pytest
import torch

import packing_cases as P
from emu_backend import emulated_backend

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


@P.params
def test_refresh_after_smaller_weights_equals_a_new_packer(spec):
    P.smaller_weights(CPU, spec)


@P.params
def test_refresh_after_moved_storage_equals_a_new_packer(spec):
    P.moved_storage(CPU, spec)


@P.params
def test_refresh_without_a_change_issues_no_call(spec):
    P.no_change_no_launch(CPU, spec)


@P.params
def test_refresh_rejects_tensors_that_are_not_contiguous_fp32(spec):
    P.rejected_tensors(CPU, spec)
