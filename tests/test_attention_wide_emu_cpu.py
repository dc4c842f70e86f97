"""The 128-channel attention parity tests of test_attention_wide_gpu.py on the CPU emulator (tools/hipemu), on small shapes: every
128-wide kernel -- generic forward on each option path, pre-split bf16x3 / fp16-pair forms, dq / dkv backward -- gets its first
correctness check without a GPU.  The `-m gpu` twin is the parity test proper."""
import pytest
import torch

import test_attention_wide_gpu as W
import test_backward_kernels_gpu as BK
import test_kernels_gpu as K
from emu_backend import emulated_backend

CPU = torch.device("cpu")
CH = 128


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emulated_backend() as emu:
        yield emu


@pytest.mark.parametrize("N,T,heads", [(2, 16, 2), (1, 100, 1), (1, 37, 2)])
@pytest.mark.parametrize("new_order", [False, True])
def test_attention(N, T, heads, new_order):
    K.test_attention(CPU, N, T, heads, CH, new_order)


@pytest.mark.parametrize("N,Tq,Tk,heads", [(1, 100, 37, 2), (1, 16, 64, 1)])
def test_cross_attention(N, Tq, Tk, heads):
    K.test_cross_attention(CPU, N, Tq, Tk, heads, CH)


@pytest.mark.parametrize("N,T,heads", [(2, 16, 2), (1, 100, 1)])
@pytest.mark.parametrize("new_order", [False, True])
def test_attention_backward(N, T, heads, new_order):
    BK.test_attention_backward(CPU, N, T, heads, CH, new_order)


@pytest.mark.parametrize("N,Tq,Tk,heads", [(1, 64, 64, 2), (1, 100, 37, 1)])
def test_cross_attention_backward(N, Tq, Tk, heads):
    BK.test_cross_attention_backward(CPU, N, Tq, Tk, heads, CH)


@pytest.mark.parametrize("N,Tq,Tk,heads", [(1, 100, 37, 1), (1, 33, 31, 1), (1, 64, 96, 1)])
def test_attention_interleaved_loop_is_bit_equal(N, Tq, Tk, heads):
    K.test_attention_interleaved_loop_is_bit_equal(CPU, N, Tq, Tk, heads, CH)


@pytest.mark.parametrize("N,T,heads,new_order", [(1, 128, 2, False), (1, 128, 1, True)])
def test_attention_presplit_form_is_bit_equal(N, T, heads, new_order):
    K.test_attention_presplit_form_is_bit_equal(CPU, N, T, heads, CH, new_order)


@pytest.mark.parametrize("N,T,heads,new_order,slack", [(1, 128, 2, False, 1.0), (1, 128, 1, True, 4096.0)])
def test_attention_h2(N, T, heads, new_order, slack):
    K.test_attention_h2(CPU, N, T, heads, CH, new_order, slack)


def test_attention_forces_rescale():
    W.check_forces_rescale(CPU)


@pytest.mark.parametrize("ch", [48, 256])
def test_other_widths_still_rejected(ch):
    W.test_other_widths_still_rejected(CPU, ch)
