"""Loss meter (csrc/loss_meter.hip, bbdm_amd/loss_meter.py, the hook in BrownianBridgeModel._denoise_and_loss) on the GPU: the cases
of tests/loss_meter_cases.py."""
import pytest
import torch

import loss_meter_cases as C

pytestmark = pytest.mark.gpu
SHAPES = pytest.mark.parametrize("per_sample,off", C.KERNEL_SHAPES, ids=C.KERNEL_IDS)
LOSS = pytest.mark.parametrize("loss_type", C.LOSS_TYPES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@SHAPES
@LOSS
@pytest.mark.parametrize("n", [1, 5])
def test_per_image_loss_is_within_one_fp32_ulp_of_float64(dev, per_sample, off, n, loss_type):
    C.per_image_values(dev, per_sample, off, n, loss_type)


@LOSS
@pytest.mark.parametrize("T,B", C.TABLES)
def test_bucket_table_counts_and_sums(dev, T, B, loss_type):
    C.bucket_table(dev, T, B, loss_type)


@LOSS
@pytest.mark.parametrize("per_sample", [75, 3072])
def test_state_is_bitwise_independent_of_order_batching_and_alignment(dev, per_sample, loss_type):
    C.order_and_batching(dev, per_sample, loss_type)


def test_out_of_range_t_is_rejected_on_the_int64_value(dev):
    C.rejected_timesteps(dev)


def test_non_finite_image_marks_its_bucket_until_reset(dev):
    C.non_finite(dev)


def test_merge_state_dict_and_table_mismatch(dev):
    C.merge_and_state_dict(dev)


def test_attaching_a_meter_changes_nothing_pixel_model(dev):
    C.attach_changes_nothing_pixel(dev)


def test_attaching_a_meter_changes_nothing_latent_model(dev):
    C.attach_changes_nothing_latent(dev)


def test_validation_loss_is_repeatable_and_equals_the_written_out_loop(dev):
    C.validation_loss_pixel(dev)


def test_validation_loss_on_cache_rows_equals_validation_loss_on_images(dev):
    C.validation_loss_latent_cache(dev)


def test_out_of_range_t_indexes_the_schedule_tables_clamped(dev):
    C.out_of_range_t_reads_no_memory_beside_the_tables(dev)
