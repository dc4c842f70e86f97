"""The first stage's own kernels (tests/first_stage_kernel_cases.py) on the GPU: the batched activation GEMM, the row softmax, the
decimating modes of bbdm_groupnorm_apply_f32 and the codebook search against fp64 references, plus the two sizes only a GPU run
reaches (the product's 4096-token q k^T and the grid-stride pass of the codebook search)."""
import pytest
import torch

import first_stage_kernel_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("batch,rows,Kd,R,transposed", K.GEMM_CASES)
def test_gemm_batched(dev, batch, rows, Kd, R, transposed):
    K.gemm_batched(dev, batch, rows, Kd, R, transposed)


def test_gemm_batched_product_size(dev):
    K.gemm_batched(dev, *K.GEMM_PRODUCT_CASE)


@pytest.mark.parametrize("rows,T,ld,xm,scale", K.SOFTMAX_CASES)
def test_softmax_rows(dev, rows, T, ld, xm, scale):
    K.softmax_rows(dev, rows, T, ld, xm, scale)


def test_softmax_uniform_row(dev):
    K.softmax_uniform_row(dev)


@pytest.mark.parametrize("N,H,W,C,groups", K.DECIMATE_CASES)
def test_decimate(dev, N, H, W, C, groups):
    K.decimate(dev, N, H, W, C, groups)


def test_decimate_rejects_odd_sizes(dev):
    K.decimate_rejects_odd_sizes(dev)


def test_strided_conv_through_decimation(dev):
    K.strided_conv_through_decimation(dev)


@pytest.mark.parametrize("e_dim,n_e,pixels,ldz,ldq", K.VQ_CASES)
def test_vq_nearest(dev, e_dim, n_e, pixels, ldz, ldq):
    K.vq_nearest(dev, e_dim, n_e, pixels, ldz, ldq)


def test_vq_nearest_grid_stride(dev):
    K.vq_nearest_grid_stride(dev)


def test_vq_nearest_rejects(dev):
    K.vq_nearest_rejects(dev)


def test_argument_checks(dev):
    K.argument_checks(dev)
