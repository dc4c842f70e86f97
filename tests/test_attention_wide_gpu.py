"""128-channel attention heads (GPU): the attention kernel parity tests of test_kernels_gpu.py / test_backward_kernels_gpu.py at
ch = 128 -- the generic forward on every path the options select, the pre-split bf16x3 and fp16-pair forms, the backward of the
packed-qkv and the cross-attention -- against the same fp64 / fp32 references and tolerances."""
import math

import pytest
import torch

import test_backward_kernels_gpu as BK
import test_kernels_gpu as K
from fixtures import rel_err

pytestmark = pytest.mark.gpu
CH = 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.mark.parametrize("N,T,heads", [(2, 16, 4), (1, 256, 2), (2, 100, 3), (2, 37, 1), (1, 1024, 8)])
@pytest.mark.parametrize("new_order", [False, True])
def test_attention(dev, N, T, heads, new_order):
    K.test_attention(dev, N, T, heads, CH, new_order)


@pytest.mark.parametrize("N,Tq,Tk,heads", [(2, 100, 37, 3), (1, 200, 77, 4), (1, 256, 1024, 2)])
def test_cross_attention(dev, N, Tq, Tk, heads):
    K.test_cross_attention(dev, N, Tq, Tk, heads, CH)


@pytest.mark.parametrize("N,T,heads", [(2, 16, 4), (2, 100, 3), (1, 300, 1), (2, 256, 8)])
@pytest.mark.parametrize("new_order", [False, True])
def test_attention_backward(dev, N, T, heads, new_order):
    BK.test_attention_backward(dev, N, T, heads, CH, new_order)


@pytest.mark.parametrize("N,Tq,Tk,heads", [(2, 64, 64, 2), (1, 200, 77, 4)])
def test_cross_attention_backward(dev, N, Tq, Tk, heads):
    BK.test_cross_attention_backward(dev, N, Tq, Tk, heads, CH)


@pytest.mark.parametrize("N,Tq,Tk,heads", [(2, 160, 160, 2), (1, 100, 37, 3), (1, 256, 1000, 2), (2, 33, 32, 1), (1, 64, 31, 2)])
def test_attention_interleaved_loop_is_bit_equal(dev, N, Tq, Tk, heads):
    K.test_attention_interleaved_loop_is_bit_equal(dev, N, Tq, Tk, heads, CH)


@pytest.mark.parametrize("N,T,heads,new_order", [(2, 128, 2, False), (1, 128, 3, True), (1, 1024, 2, False), (2, 1024, 1, True)])
def test_attention_presplit_form_is_bit_equal(dev, N, T, heads, new_order):
    K.test_attention_presplit_form_is_bit_equal(dev, N, T, heads, CH, new_order)


@pytest.mark.parametrize("N,T,heads,new_order,slack", [(2, 128, 2, False, 1.0), (1, 256, 3, True, 4096.0), (1, 1024, 2, False, 1.0),
                                                       (1, 4096, 2, False, 4096.0)])     # (the last: C2's sequence length)
def test_attention_h2(dev, N, T, heads, new_order, slack):
    K.test_attention_h2(dev, N, T, heads, CH, new_order, slack)


def check_forces_rescale(dev, ch=CH):
    """test_kernels_gpu.py::test_attention_forces_rescale at another head width: a key whose score dwarfs all earlier ones appears in the
    last key tile, so the online-softmax rescale branch runs there, on every forward path the options select."""
    from bbdm_amd import _lib
    import kernel_ops as ops
    g = torch.Generator().manual_seed(3)
    N, T, heads = 1, 160, 1
    qkv = torch.randn(N, 3 * ch, T, generator=g)
    qkv[0, ch:2 * ch, 150] = qkv[0, :ch, 7] * 6.0          # k_150 aligned with q_7 -> huge score in the last tile
    q, k, v = qkv.reshape(1, 3 * ch, T).split(ch, dim=1)
    s = 1 / math.sqrt(math.sqrt(ch))
    wgt = torch.softmax(torch.einsum("bct,bcs->bts", (q * s).double(), (k * s).double()), dim=-1)
    ref = torch.einsum("bts,bcs->bct", wgt, v.double()).float()
    x = qkv.permute(0, 2, 1).contiguous().to(dev)
    for bf3, pipe in ((1, 1), (1, 0), (2, 0), (0, 0)):
        with _lib.option("attn_bf3", bf3), _lib.option("attn_pipe", pipe):
            out = ops.attention(x, heads)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert rel_err(out.cpu().permute(0, 2, 1), ref) < K.TOL, (bf3, pipe)


def test_attention_forces_rescale(dev):
    check_forces_rescale(dev)


@pytest.mark.parametrize("ch", [48, 96, 256])
def test_other_widths_still_rejected(dev, ch):
    """Widths outside {16, 32, 64, 128} are refused by every entry point, forward and backward; no pre-split form for them."""
    from bbdm_amd import _lib
    import kernel_ops as ops
    lib = _lib.load()
    qkv = torch.randn(1, 64, 3 * ch, device=dev)
    with pytest.raises(_lib.BBDMHipError, match="head channels"):
        ops.attention(qkv, 1)
    q = torch.randn(1, 64, ch, device=dev)
    with pytest.raises(_lib.BBDMHipError, match="head channels"):
        ops.cross_attention(q, q, q, 1)
    assert lib.bbdm_attention_kv_planes_bytes(1, 1024, 1, ch) == 0 and lib.bbdm_attention_kv_planes_h2_bytes(1, 1024, 1, ch) == 0
    out, lse = torch.zeros(1, 64, ch, device=dev), torch.zeros(64, device=dev)
    with pytest.raises(_lib.BBDMHipError, match="bad shape"):
        ops.attention_bwd(qkv, out, out, lse, 1, False)
