"""Weight packing (bbdm_amd/packing.py) on the GPU: the one refresh protocol over every packer and plane layout the planner can
construct, bit for bit -- and on a second stream, where the training plan re-packs its data-gradient operands."""
import pytest
import torch

import packing_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@P.params
def test_refresh_after_smaller_weights_equals_a_new_packer(dev, spec):
    P.smaller_weights(dev, spec)


@P.params
def test_refresh_after_moved_storage_equals_a_new_packer(dev, spec):
    P.moved_storage(dev, spec)


@P.params
def test_refresh_without_a_change_issues_no_call(dev, spec):
    P.no_change_no_launch(dev, spec)


@P.params
def test_refresh_rejects_tensors_that_are_not_contiguous_fp32(dev, spec):
    P.rejected_tensors(dev, spec)


@P.params
def test_refresh_on_a_second_stream_equals_the_current_stream(dev, spec):
    P.second_stream(dev, spec)
