"""The first stage's own kernels (tests/first_stage_kernel_cases.py) on the CPU-emulated HIP kernels."""
import pytest
import torch

import first_stage_kernel_cases as K
from emu_backend import emulated_backend

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


@pytest.mark.parametrize("batch,rows,Kd,R,transposed", K.GEMM_CASES)
def test_gemm_batched(batch, rows, Kd, R, transposed):
    K.gemm_batched(CPU, batch, rows, Kd, R, transposed)


@pytest.mark.parametrize("rows,T,ld,xm,scale", K.SOFTMAX_CASES)
def test_softmax_rows(rows, T, ld, xm, scale):
    K.softmax_rows(CPU, rows, T, ld, xm, scale)


def test_softmax_uniform_row():
    K.softmax_uniform_row(CPU)


@pytest.mark.parametrize("N,H,W,C,groups", K.DECIMATE_CASES)
def test_decimate(N, H, W, C, groups):
    K.decimate(CPU, N, H, W, C, groups)


def test_decimate_rejects_odd_sizes():
    K.decimate_rejects_odd_sizes(CPU)


def test_strided_conv_through_decimation():
    K.strided_conv_through_decimation(CPU)


@pytest.mark.parametrize("e_dim,n_e,pixels,ldz,ldq", K.VQ_CASES)
def test_vq_nearest(e_dim, n_e, pixels, ldz, ldq):
    K.vq_nearest(CPU, e_dim, n_e, pixels, ldz, ldq)


def test_vq_nearest_rejects():
    K.vq_nearest_rejects(CPU)


def test_argument_checks():
    K.argument_checks(CPU)
