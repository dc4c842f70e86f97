"""Weight packing: everything that turns an ``nn.Parameter`` into the device operands the kernels read.

One refresh protocol (:class:`_Packed`: key on the storage and version of what the packer reads, check it, re-pack, store the key)
and one description of the matrix-core plane layouts (:class:`_Planes`), shared by the 1x1 / direct packer (:class:`_PackedConv`),
the Winograd packer (:class:`_PackedWinograd`) and the row-L1 gain (:class:`_RowL1Gain`).  Which layer takes which packer and
layout is the planner's business (bbdm_amd/unet.py); so are the Winograd tile policies.

The library is reached as ``_lib.call`` / ``_lib.load`` only: the CPU emulator of the tests swaps attributes of that module.
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch
import torch.nn as nn

from . import _lib


class _NoVersion:
    """Stands in for the version of a tensor that has no version counter: never equal to anything.  (A FRESH instance per read:
    container comparisons short-cut on identity.)"""

    def __eq__(self, other):
        return False

    __hash__ = object.__hash__


def _ver(t: torch.Tensor):
    """``t._version``, or a :class:`_NoVersion` for inference tensors (``torch.inference_mode()``: no version counter).  The version
    only tracks writes made through torch ops on ``t`` or its views -- a raw-pointer kernel or a DLPack consumer does not bump it --
    so every cache keyed on it must tolerate a miss: a key containing a ``_NoVersion`` never matches, i.e. the copy / re-pack runs."""
    if t.is_inference():
        return _NoVersion()
    try:
        return t._version
    except RuntimeError:
        return _NoVersion()


@contextlib.contextmanager
def _on_stream(t: torch.Tensor, stream):
    """Torch ops on ``t``'s device inside this block -- fills, and allocations, whose reuse the caching allocator orders on the stream
    that is current when they are made -- go to the raw HIP stream ``stream``: the stream the packing launches around them are given.
    (The training plans re-pack their data-gradient operands on the plan's SECOND stream; a plain torch op would go to torch's
    current stream and race with those launches.)  Nothing to switch for a CPU tensor or a null stream (the emulator's)."""
    if t.is_cuda and stream:
        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=t.device)):
            yield
    else:
        yield


def _zero_on(t: torch.Tensor, stream):
    """``t.zero_()`` enqueued on the raw HIP stream ``stream``."""
    with _on_stream(t, stream):
        t.zero_()


def wino_planes(m: int) -> int:
    """Transform points of Winograd tile ``m``: (m + 2)^2 for F(m x m, 3x3); m = 7 is F(7x7, 2x2) on the 8-point transform."""
    return 64 if m == 7 else (m + 2) ** 2


class _Packed:
    """Device buffers derived from one weight (and, where the packer reads it, its bias), re-packed when the storage or the version
    of a tensor it reads changes (EMA swaps ``param.data`` without bumping ``_version`` -- runners/base/EMA.py:31-43 -- so both are
    keyed).  Subclasses implement ``_pack(stream)``."""

    def __init__(self, weight: nn.Parameter, bias: Optional[nn.Parameter] = None, reads_bias: bool = False):
        self.weight, self.bias = weight, bias
        self._reads = (weight,) if bias is None or not reads_bias else (weight, bias)
        self.key = None

    def refresh(self, stream):
        key = tuple((t.data_ptr(), _ver(t)) for t in self._reads)
        if key != self.key:
            for t in self._reads:       # (the pack kernels take raw pointers)
                if not t.is_contiguous() or t.dtype != torch.float32:
                    raise RuntimeError("bbdm_amd: conv weights must be contiguous fp32")
            self._pack(stream)
            self.key = key

    def _pack(self, stream):
        raise NotImplementedError


# plane layout (the planner's mode value) -> (size query, element type, split entry point); False = the fp32 packing is the operand
_LAYOUTS = {
    True: ("bbdm_gemm_bf3_packed_halfs", torch.int16, "bbdm_gemm_bf3_pack_f32"),        # three bf16 planes, csrc/gemm_bf3.hip
    "p": ("bbdm_gemm_bf3p_b_bytes", torch.uint8, "bbdm_gemm_bf3p_pack_b_f32"),          # ... in fragment units, csrc/gemm_bf3p.hip
    "h": ("bbdm_gemm_h2p_b_bytes", torch.uint8, "bbdm_gemm_h2p_pack_b_f32"),            # two fp16 planes under ``ubound``, csrc/h2_split.h
}


class _Planes:
    """The B operand [planes][K][N] of a matrix-core GEMM in one of the layouts above: ``packed``, and for "h" the device float
    ``ubound`` that bounds the fp32 values the planes are split from."""

    def __init__(self, layout, planes: int, K: int, N: int, device):
        size, dtype, self.entry = _LAYOUTS[layout]
        self.dims = (planes, K, N)
        self.packed = torch.empty(getattr(_lib.load(), size)(planes, K, N), dtype=dtype, device=device)
        self.ubound = torch.zeros(1, dtype=torch.float32, device=device) if layout == "h" else None

    def measure(self, src: torch.Tensor, stream):
        """``ubound`` = max |src| (zeroed on ``stream`` first: the kernel accumulates a maximum)."""
        _zero_on(self.ubound, stream)
        _lib.call("bbdm_absmax_f32", src.data_ptr(), src.numel(), self.ubound.data_ptr(), stream)

    def split(self, src: torch.Tensor, stream, gain: float = 1.0, measure: bool = True):
        """Split the fp32 packing ``src`` into the planes.  "h": under ``gain`` x ``ubound``, where ``ubound`` is the maximum of ``src``
        itself unless the caller has measured it already (``measure`` False: the Winograd packer bounds the taps, not G g G^T)."""
        if self.ubound is None:
            _lib.call(self.entry, src.data_ptr(), self.packed.data_ptr(), *self.dims, stream)
            return
        if measure:
            self.measure(src, stream)
        _lib.call(self.entry, src.data_ptr(), self.packed.data_ptr(), self.ubound.data_ptr(), gain, *self.dims, stream)


class _PackedConv(_Packed):
    """Packed copy of one conv / Linear weight for the direct kernel -- ``dgrad``: transposed + flipped, so that the forward kernel run
    with it computes the data gradient dX = dY W (``pad`` is then the padded Cout the gradient arrives with, else the padded Cin).
    With a plane ``layout`` (1x1 layers) that fp32 packing is the intermediate and ``packed`` the matrix-core operand of
    bbdm_conv1x1_bf3_f32 (True), _bf3q / _bf3s ("p") or _h2q / _h2s ("h": under the scale of its exact maximum ``ubound``)."""

    def __init__(self, weight: nn.Parameter, bias: Optional[nn.Parameter], pad: int, layout=False, dgrad: bool = False):
        super().__init__(weight, bias)
        self.cout, self.cin = weight.shape[0], weight.shape[1]
        self.ks = weight.shape[2] if weight.dim() == 4 else 1      # Conv1d k=1: [O, I, 1] == [O, I, 1, 1] in memory
        self.pad, self.dgrad = pad, dgrad
        lib = _lib.load()
        n = lib.bbdm_conv_packed_dgrad_floats(self.cout, self.cin, pad, self.ks) if dgrad else lib.bbdm_conv_packed_floats(self.cout, pad, self.ks)
        self.packed_f32 = self.packed = torch.empty(n, dtype=torch.float32, device=weight.device)
        self.planes = self.ubound = None
        if layout:
            assert self.ks == 1
            self.planes = _Planes(layout, 1, pad, self.cin if dgrad else self.cout, weight.device)
            self.packed, self.ubound = self.planes.packed, self.planes.ubound
        if not dgrad:
            self.packed.cin_true = self.cin          # algorithmic (unpadded) input channels, for flop accounting

    def _pack(self, stream):
        _lib.call("bbdm_conv_pack_weight_dgrad_f32" if self.dgrad else "bbdm_conv_pack_weight_f32", self.weight.data_ptr(),
                  self.packed_f32.data_ptr(), self.cout, self.cin, self.pad, self.ks, stream)
        if self.planes is not None:
            self.planes.split(self.packed_f32, stream)


class _RowL1Gain(_Packed):
    """(max over rows of sum |W[row, :]|, max |bias|) of a 1x1 conv / Linear as two device floats, refreshed with the weights: what
    turns a bound of the layer's input into a bound of its output (csrc/groupnorm.hip: h2_rowl1_kernel / bbdm_h2_affine_bound_f32)."""

    def __init__(self, weight, bias):
        super().__init__(weight, bias, reads_bias=True)
        self.gain = torch.zeros(2, dtype=torch.float32, device=weight.device)

    def _pack(self, stream):
        w, b = self.weight, self.bias
        _lib.call("bbdm_h2_rowl1_f32", w.data_ptr(), None if b is None else b.data_ptr(), w.shape[0], w[0].numel(),
                  self.gain.data_ptr(), stream)


class _PackedWinograd(_Packed):
    """G g G^T of one 3x3 conv weight in the batched-GEMM layout (``dgrad``: of the data-gradient convolution).  With
    ``bf3`` the fp32 tensor is split into a plane layout and ``packed`` is that operand: True = the three bf16 planes of
    csrc/gemm_bf3.hip (the op binds to bbdm_winograd_gemm_bf3_f32), "p" = the planes in the fragment-unit layout of
    csrc/gemm_bf3p.hip, whose A operand the input transform writes pre-split (bbdm_winograd_input_bf3p_f32 / _gemm_bf3p_f32),
    "h" = two fp16 planes of U 2^e (csrc/h2_split.h): e from ``ubound`` = the filter's largest tap times the gain of G . G^T, the
    factor the tile GEMM applies to the same pointer.

    ``phases``: the layer is conv3x3(nearest x2 (x)); packed are its four phase filters, a conv Cin -> 4 Cout on x itself
    (bbdm_upsample_phase_weights_f32, BBDM_CONV_OUT_PHASES).

    The fp32 G g G^T tensor (4x the weights at m = 4) is kept only where it is the operand or feeds a split on every re-pack.  The
    phase filters on the fp16 pair have no single-launch kernel and take it as a TRANSIENT scratch from torch's allocator, inside
    :func:`_on_stream`: every launch that touches it goes to ``refresh``'s raw stream, so that is the stream the allocator must order
    its reuse on -- whichever list of the plan (the side-stream ``dconvs`` included) such a packer is ever put in."""

    def __init__(self, weight: nn.Parameter, bias: Optional[nn.Parameter], in_pad: int, m: int, dgrad: bool = False,
                 bf3=False, phases: bool = False):
        super().__init__(weight, bias)
        self.dgrad, self.m, self.bf3, self.phases = dgrad, m, bf3, phases
        self.cout, self.cin = weight.shape[0], weight.shape[1]
        self.ks, self.in_pad = 3, in_pad
        assert not (phases and dgrad)
        dev = weight.device
        self.w4 = torch.empty(4 * self.cout, self.cin, 3, 3, dtype=torch.float32, device=dev) if phases else None
        self.out_ch = self.cin if dgrad else (4 * self.cout if phases else self.cout)
        self._n_f32 = _lib.load().bbdm_winograd_packed_floats(m, self.out_ch, in_pad)
        # single-launch kernels write the planes straight from the weights ("h": see _pack)
        self.fused_planes = bf3 == "p" and not phases and in_pad % 16 == 0
        self.packed_f32 = None if (self.fused_planes or bf3 == "h") else torch.empty(self._n_f32, dtype=torch.float32, device=dev)
        self.planes = _Planes(bf3, wino_planes(m), in_pad, self.out_ch, dev) if bf3 else None
        self.packed = self.planes.packed if bf3 else self.packed_f32
        self.ubound = self.planes.ubound if bf3 else None
        self.packed.cin_true = self.cout if dgrad else self.cin

    def _pack(self, stream):
        w, h2, dg = self.weight, self.bf3 == "h", 1 if self.dgrad else 0
        src, n_out = w, self.cout
        if self.phases:
            _lib.call("bbdm_upsample_phase_weights_f32", w.data_ptr(), self.w4.data_ptr(), self.cout, self.cin, stream)
            src, n_out = self.w4, 4 * self.cout
        if h2:
            self.planes.measure(src, stream)        # the largest tap: one small pass over the weights
        # G g G^T straight into the planes where one launch does it (no fp32 tensor in between)
        if h2 and not self.phases:
            _lib.call("bbdm_winograd_pack_weight_h2p_f32", self.m, w.data_ptr(), self.packed.data_ptr(), self.cout, self.cin,
                      self.in_pad, dg, self.ubound.data_ptr(), stream)
            return
        if self.fused_planes:
            _lib.call("bbdm_winograd_pack_weight_bf3p_f32", self.m, w.data_ptr(), self.packed.data_ptr(), self.cout, self.cin,
                      self.in_pad, dg, stream)
            return
        # ... otherwise fp32 G g G^T, then the split
        u = self.packed_f32
        if u is None:
            with _on_stream(w, stream):
                u = torch.empty(self._n_f32, dtype=torch.float32, device=w.device)
        _lib.call("bbdm_winograd_pack_weight_f32", self.m, src.data_ptr(), u.data_ptr(), n_out, self.cin, self.in_pad, dg, stream)
        if self.planes is not None:
            self.planes.split(u, stream, gain=float(_lib.load().bbdm_winograd_g_gain(self.m)) if h2 else 1.0, measure=False)
