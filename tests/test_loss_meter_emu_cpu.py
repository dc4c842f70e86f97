"""Loss meter (csrc/loss_meter.hip, bbdm_amd/loss_meter.py, the hook in BrownianBridgeModel._denoise_and_loss) on the CPU-emulated
kernels (tools/hipemu): the product code paths with every launch executed by the emulator.  The rejected-t case runs here before it
runs on a device.  The two cases on the tiny latent model run on
the GPU only: one emulated training step of that model takes a quarter of a minute."""
import pytest
import torch

import loss_meter_cases as C
from emu_backend import emulated_backend

CPU = torch.device("cpu")
SHAPES = pytest.mark.parametrize("per_sample,off", C.KERNEL_SHAPES, ids=C.KERNEL_IDS)
LOSS = pytest.mark.parametrize("loss_type", C.LOSS_TYPES)


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


@SHAPES
@LOSS
@pytest.mark.parametrize("n", [1, 5])
def test_per_image_loss_is_within_one_fp32_ulp_of_float64(per_sample, off, n, loss_type):
    C.per_image_values(CPU, per_sample, off, n, loss_type)


@LOSS
@pytest.mark.parametrize("T,B", C.TABLES)
def test_bucket_table_counts_and_sums(T, B, loss_type):
    C.bucket_table(CPU, T, B, loss_type)


@LOSS
@pytest.mark.parametrize("per_sample", [75, 3072])
def test_state_is_bitwise_independent_of_order_batching_and_alignment(per_sample, loss_type):
    C.order_and_batching(CPU, per_sample, loss_type)


def test_out_of_range_t_is_rejected_on_the_int64_value():
    C.rejected_timesteps(CPU)


def test_non_finite_image_marks_its_bucket_until_reset():
    C.non_finite(CPU)


def test_merge_state_dict_and_table_mismatch():
    C.merge_and_state_dict(CPU)


def test_attaching_a_meter_changes_nothing_pixel_model():
    C.attach_changes_nothing_pixel(CPU)


def test_validation_timesteps_match_the_formula_in_python_integers():
    C.validation_timesteps_match_the_formula()


def test_validation_loss_is_repeatable_and_equals_the_written_out_loop():
    C.validation_loss_pixel(CPU)


def test_out_of_range_t_indexes_the_schedule_tables_clamped():
    C.out_of_range_t_reads_no_memory_beside_the_tables(CPU)
