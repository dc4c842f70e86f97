#!/usr/bin/env python
"""Old library against new, bit for bit:  python tools/lib_ab.py OLD.so NEW.so [--emu]

For refactors of the launchers in bbdm_amd/csrc: both builds must route every call to the same kernel instance with the same grid,
so every output buffer must come out with the same bits.  One fresh child process per library (one after the other; nothing is
started after a child fails, each under its own time limit) runs the same seeded grid of direct C-ABI calls and writes a SHA-256 per
output buffer; the parent compares the two lists, prints the first call that differs with its arguments and exits non-zero.

GPU builds: the child runs with BBDM_HIP_LIB = the library.  --emu: both are builds of tools/hipemu (CPU tensors), bound with
_lib.bind(path).  The grid is the product of each launcher's routing conditions at the smallest shapes that reach the route; a call
that the library rejects is recorded with its error text (and must be rejected alike by both).  Routes that differ only in index
width give equal bits by design and are run all the same: a wrong route that leaves its buffers shows on the emulator's bounds.
The elementwise files (bridge.hip, optim.hip, loss_meter.hip; built without FMA contraction, so a refactor of their KERNELS keeps every
bit as well) are covered entry point by entry point: elementwise_grid().
"""
import argparse
import ctypes
import hashlib
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 900          # seconds per library


class Rejected(Exception):
    """The library refused the call (rc != 0 with its error text): a result like any other, which both builds must give alike."""


class Ctx:
    def __init__(self, lib, dev):
        import torch
        self.torch, self.lib, self.dev = torch, lib, dev
        self.st = None if dev == "cpu" else torch.cuda.current_stream().cuda_stream

    def rand(self, seed, *shape, scale=1.0):
        g = self.torch.Generator().manual_seed(seed)
        return (self.torch.randn(*shape, generator=g, dtype=self.torch.float32) * scale).to(self.dev)

    def zeros(self, n, dtype=None):
        return self.torch.zeros(int(n), dtype=dtype or self.torch.float32, device=self.dev)

    def bytes_(self, n):
        return self.torch.zeros(int(n) + 64, dtype=self.torch.uint8, device=self.dev)

    def scalar(self, v):
        return self.torch.full((1,), float(v), dtype=self.torch.float32, device=self.dev)

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            msg = self.lib.bbdm_last_error()
            raise Rejected(f"{name}: rc={rc}: {msg.decode() if msg else ''}")

    def option(self, name, value):
        self.call("bbdm_set_option", name.encode(), int(value))


def P(t):
    return None if t is None else t.data_ptr()


def planes_of(m):
    return 64 if m == 7 else (m + 2) ** 2


def hw_of(m, ragged=False):
    """Two tiles per side (one ragged for m >= 6 when asked); even, so that upsample = 1 passes."""
    return 2 * m - 2 if ragged and m >= 6 else (14 if m == 7 else 2 * m)


# ---- the cases: each yields (name, args dict, function(ctx) -> list of output tensors) ---------------------------------------------------
INPUT_FORMS = ("f32_thread", "f32_rows", "bf3p", "bf3p_tr", "bf3p_gn", "h2p", "h2p_tr", "h2p_tr2", "h2p_gn")


def input_case(c, m, pre, up, form, idx64, ragged):
    N, H = 2, hw_of(m, ragged)
    W = H
    cin = 24 if form == "f32_thread" else 32
    pl = planes_of(m)
    tiles = c.lib.bbdm_winograd_tiles(m, N, H, W)
    c.option("wino_idx64", idx64)
    try:
        x = c.rand(1, N, H // 2 if up else H, W // 2 if up else W, cin)
        sc = c.rand(2, N, cin) if pre else None
        bi = c.rand(3, N, cin) if pre else None
        pa = (P(sc), P(bi), cin if pre else 0, 1 if pre else 0)
        bound = c.scalar(8.0)
        outs = []
        if form.startswith("f32"):
            V = c.zeros(pl * tiles * cin)
            c.call("bbdm_winograd_input_f32", m, P(x), cin, P(V), *pa, up, N, H, W, cin, c.st)
            return [V]
        h2 = form.startswith("h2p")
        Vp = c.bytes_((c.lib.bbdm_gemm_h2p_a_bytes if h2 else c.lib.bbdm_gemm_bf3p_a_bytes)(pl, tiles, cin))
        outs.append(Vp)
        if form.endswith("_gn"):
            G = 4
            stats = c.zeros(c.lib.bbdm_groupnorm_stats_bytes(N, G) // 8, c.torch.int64)
            c.call("bbdm_groupnorm_stats_f32", P(x), cin, P(stats), N, x.shape[1] * x.shape[2], cin, G, c.st)
            gamma, beta = c.rand(4, cin), c.rand(5, cin)
            film = c.rand(6, N, 2 * cin) if pre else None
            tail = (P(gamma), P(beta), P(film), 2 * cin if pre else 0, x.shape[1] * x.shape[2], G, 1e-5)
            if h2:
                c.call("bbdm_winograd_input_h2p_gn_f32", m, P(x), cin, P(Vp), P(stats), None, cin, 1, up, N, H, W, cin, *tail, P(bound), c.st)
            else:
                c.call("bbdm_winograd_input_bf3p_gn_f32", m, P(x), cin, P(Vp), P(stats), None, cin, 1, up, N, H, W, cin, *tail, c.st)
        elif "_tr" in form:
            tr2 = form == "h2p_tr2"
            Vt = c.bytes_((c.lib.bbdm_gemm_h2p_tn_at_bytes if tr2 else c.lib.bbdm_gemm_bf3p_tn_at_bytes)(pl, tiles, cin))
            outs.append(Vt)
            if h2:
                c.call("bbdm_winograd_input_" + form + "_f32", m, P(x), cin, P(Vp), *pa, up, N, H, W, cin, P(Vt), P(bound), c.st)
            else:
                c.call("bbdm_winograd_input_bf3p_tr_f32", m, P(x), cin, P(Vp), *pa, up, N, H, W, cin, P(Vt), c.st)
        elif h2:
            c.call("bbdm_winograd_input_h2p_f32", m, P(x), cin, P(Vp), *pa, up, N, H, W, cin, P(bound), c.st)
        else:
            c.call("bbdm_winograd_input_bf3p_f32", m, P(x), cin, P(Vp), *pa, up, N, H, W, cin, c.st)
        return outs
    finally:
        c.option("wino_idx64", 0)


def output_case(c, m, cout, res, nstats, cpg, splits, phases, shape):
    """shape: "two" tiles per side, "one" tile per image (tpw = 1), "ragged" (m >= 6), "wide" (enough workgroups for tpw > 2)."""
    N = 2
    H = {"two": hw_of(m), "one": 7 if m == 7 else m, "ragged": hw_of(m, True), "wide": 112}[shape]
    W = H
    tiles = c.lib.bbdm_winograd_tiles(m, N, H, W)
    cm = 4 * cout if phases else cout
    M = c.rand(11, splits * planes_of(m) * tiles * cm)
    bias = c.rand(12, cout)
    flags = (8 if phases else 0) | {"none": 0, "image": 2, "up": 4}[res]      # BBDM_CONV_OUT_PHASES, _RES_PER_IMAGE, _RES_UPSAMPLE
    oh, ow = (2 * H, 2 * W) if phases else (H, W)
    r = None if res == "none" else c.rand(13, N, cout) if res == "image" else c.rand(13, N, H // 2, W // 2, cout)
    out = c.zeros(N * oh * ow * cout)
    st = [c.zeros(c.lib.bbdm_groupnorm_stats_bytes(N, 32) // 8, c.torch.int64) if i < nstats else None for i in range(2)]   # (32 groups)
    c.call("bbdm_winograd_output_splitk_stats_f32", m, P(M), P(bias), P(r), cout if r is not None else 0, P(out), cout, flags, N, H, W, cout,
           P(st[0]), cpg if st[0] is not None else 0, 0, P(st[1]), cpg if st[1] is not None else 0, 0, splits, c.st)
    return [out] + [s for s in st if s is not None]


def pack_case(c, m, dgrad, form):
    cout, cin = (128, 16) if m == 7 else (40, 16)         # m = 7: the 4 C phase filters
    w = c.rand(21, cout, cin, 3, 3)
    if m == 7:
        w4 = c.zeros(4 * cout * cin * 9)
        c.call("bbdm_upsample_phase_weights_f32", P(w), P(w4), cout, cin, c.st)
        w, cout = w4, 4 * cout
    inpad = 48
    O, pl = (cin if dgrad else cout), planes_of(m)
    if form == "f32":
        out = c.zeros(c.lib.bbdm_winograd_packed_floats(m, O, inpad))
        c.call("bbdm_winograd_pack_weight_f32", m, P(w), P(out), cout, cin, inpad, dgrad, c.st)
    elif form == "bf3p":
        out = c.bytes_(c.lib.bbdm_gemm_bf3p_b_bytes(pl, inpad, O))
        c.call("bbdm_winograd_pack_weight_bf3p_f32", m, P(w), P(out), cout, cin, inpad, dgrad, c.st)
    else:
        out, bound = c.bytes_(c.lib.bbdm_gemm_h2p_b_bytes(pl, inpad, O)), c.scalar(8.0)
        c.call("bbdm_winograd_pack_weight_h2p_f32", m, P(w), P(out), cout, cin, inpad, dgrad, P(bound), c.st)
    return [out]


def dy_case(c, m, h2):
    N, H, cout = 2, hw_of(m, True), 40
    W = H
    tiles = c.lib.bbdm_winograd_tiles(m, N, H, W)
    dy = c.rand(31, N, H, W, cout)
    dMt = c.bytes_((c.lib.bbdm_gemm_h2p_tn_bt_bytes if h2 else c.lib.bbdm_gemm_bf3p_tn_bt_bytes)(planes_of(m), tiles, cout))
    dm11, bound = c.zeros(tiles * cout), c.scalar(8.0)
    if h2:
        c.call("bbdm_winograd_dy_transform_h2p_f32", m, P(dy), cout, P(dMt), P(dm11), N, H, W, cout, P(bound), c.st)
    else:
        c.call("bbdm_winograd_dy_transform_bf3p_f32", m, P(dy), cout, P(dMt), P(dm11), N, H, W, cout, c.st)
    return [dMt, dm11]


def transform_1d_case(c, m, which):
    fn = c.lib.bbdm_debug_winograd_transform_1d          # a host function: plain arrays
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    src = c.torch.arange(1, 17, dtype=c.torch.float32).sin()
    dst = c.torch.zeros(16, dtype=c.torch.float32)
    rc = fn(m, which, src.data_ptr(), dst.data_ptr())
    if rc != 0:
        raise Rejected(f"transform_1d: rc={rc}: {c.lib.bbdm_last_error().decode()}")
    return [dst]


def attention_case(c, ch, bf3, pipe, new_order, form, T):
    """form: "fwd" (bbdm_attention_f32), "cross", "planes" (kv planes + attention on them), "planes_h2" (the same under a bound)."""
    N, heads = 2, 2
    C = heads * ch
    c.option("attn_bf3", bf3)
    c.option("attn_pipe", pipe)
    try:
        qkv = c.rand(41, N, T, 3 * C)
        out, lse = c.zeros(N * T * C), c.zeros(N * heads * T)
        if form == "fwd":
            c.call("bbdm_attention_f32", P(qkv), 3 * C, P(out), C, P(lse), N, T, heads, ch, new_order, c.st)
            return [out, lse]
        if form == "cross":
            q, k, v = c.rand(42, N, T, C), c.rand(43, N, 40, C), c.rand(44, N, 40, C)
            c.call("bbdm_cross_attention_f32", P(q), C, P(k), P(v), C, P(out), C, P(lse), N, T, 40, heads, ch, c.st)
            return [out, lse]
        h2 = form == "planes_h2"
        nbytes = (c.lib.bbdm_attention_kv_planes_h2_bytes if h2 else c.lib.bbdm_attention_kv_planes_bytes)(N, T, heads, ch)
        planes, bound = c.bytes_(nbytes), c.scalar(8.0)
        if h2:
            c.call("bbdm_attention_kv_planes_h2_f32", P(qkv), 3 * C, P(planes), nbytes, N, T, heads, ch, new_order, P(bound), c.st)
            c.call("bbdm_attention_planes_h2_f32", P(qkv), 3 * C, P(out), C, P(lse), N, T, heads, ch, new_order, P(planes), P(bound), c.st)
        else:
            c.call("bbdm_attention_kv_planes_f32", P(qkv), 3 * C, P(planes), nbytes, N, T, heads, ch, new_order, c.st)
            c.call("bbdm_attention_planes_f32", P(qkv), 3 * C, P(out), C, P(lse), N, T, heads, ch, new_order, P(planes), c.st)
        return [planes, out, lse]
    finally:
        c.option("attn_bf3", 1)
        c.option("attn_pipe", 2)


def attention_bwd_case(c, ch, new_order):
    N, heads, T = 1, 2, 160
    C = heads * ch
    qkv, dout = c.rand(51, N, T, 3 * C), c.rand(52, N, T, C)
    out, lse = c.zeros(N * T * C), c.zeros(N * heads * T)
    c.call("bbdm_attention_f32", P(qkv), 3 * C, P(out), C, P(lse), N, T, heads, ch, new_order, c.st)
    work, dqkv = c.zeros(N * heads * T), c.zeros(N * T * 3 * C)
    c.call("bbdm_attention_bwd_f32", P(qkv), 3 * C, P(out), C, P(dout), C, P(lse), P(work), P(dqkv), 3 * C, N, T, heads, ch, new_order, c.st)
    return [dqkv]


def vq_case(c, e_dim):
    pix, n_e = 300, 1100                                  # two codebook chunks, a ragged last block
    z, cb = c.rand(61, pix, e_dim), c.rand(62, n_e, e_dim)
    idx, zq = c.zeros(pix, c.torch.int64), c.zeros(pix * e_dim)
    c.call("bbdm_vq_nearest_f32", P(z), e_dim, P(cb), P(idx), P(zq), e_dim, pix, n_e, e_dim, c.st)
    return [idx, zq]


def tile_gemm_case(c, variant, np_, res, cout, T, cin=64):
    batch = 2
    c.option("bf3p_kernel", variant)
    try:
        x, w = c.rand(71, batch * T, cin), c.rand(72, batch, cin // 16 * (-(-cout // 128) * 128) * 16, scale=0.1)
        bias = c.rand(73, cout)
        r = c.rand(74, batch * T, cout) if res else None
        M = c.zeros(batch * T * cout)
        bound = c.scalar(8.0)
        if np_ == 3:
            a = c.bytes_(c.lib.bbdm_gemm_bf3p_a_bytes(batch, T, cin))
            b = c.bytes_(c.lib.bbdm_gemm_bf3p_b_bytes(batch, cin, cout))
            c.call("bbdm_gemm_bf3p_split_rows_f32", P(x), cin, P(a), batch, T, cin, c.st)
            c.call("bbdm_gemm_bf3p_pack_b_f32", P(w), P(b), batch, cin, cout, c.st)
            c.call("bbdm_gemm_bf3p_f32", P(a), P(b), P(bias), P(r), cout, P(M), cout, batch, T, cin, cout, c.st)
        else:
            a = c.bytes_(c.lib.bbdm_gemm_h2p_a_bytes(batch, T, cin))
            b = c.bytes_(c.lib.bbdm_gemm_h2p_b_bytes(batch, cin, cout))
            c.call("bbdm_gemm_h2p_split_rows_f32", P(x), cin, P(a), P(bound), batch, T, cin, c.st)
            c.call("bbdm_gemm_h2p_pack_b_f32", P(w), P(b), P(bound), 1.0, batch, cin, cout, c.st)
            c.call("bbdm_gemm_h2p_f32", P(a), P(b), P(bound), P(bound), P(bias), P(r), cout, P(M), cout, batch, T, cin, cout, c.st)
        return [M]
    finally:
        c.option("bf3p_kernel", 6)


def small_1x1_case(c, h2, res):
    pix, cin, cout = 200, 64, 40
    x, w, bias = c.rand(81, pix, cin), c.rand(82, cin // 16 * 128 * 16, scale=0.1), c.rand(83, cout)
    r = c.rand(84, pix, cout) if res else None
    out, bound = c.zeros(pix * cout), c.scalar(8.0)
    if h2:
        b = c.bytes_(c.lib.bbdm_gemm_h2p_b_bytes(1, cin, cout))
        c.call("bbdm_gemm_h2p_pack_b_f32", P(w), P(b), P(bound), 1.0, 1, cin, cout, c.st)
        c.call("bbdm_conv1x1_h2s_f32", P(x), cin, P(b), P(bias), P(r), cout, P(out), cout, pix, cin, cout, P(bound), P(bound), c.st)
    else:
        b = c.bytes_(c.lib.bbdm_gemm_bf3p_b_bytes(1, cin, cout))
        c.call("bbdm_gemm_bf3p_pack_b_f32", P(w), P(b), 1, cin, cout, c.st)
        c.call("bbdm_conv1x1_bf3s_f32", P(x), cin, P(b), P(bias), P(r), cout, P(out), cout, pix, cin, cout, c.st)
    return [out]


def conv_case(c, kind, stats, pre):
    """kind "stem": CinPad 8 / 4 -> 128 channels; "narrow3/4/8": a few output channels, small (8 x 8 tiles) and large images."""
    if kind.startswith("stem"):
        N, H, W, cinp, cout = 1, 64, 64, int(kind[4:]), 128
    else:
        N, cinp, cout = 1, 16, {"3": 3, "4": 4, "8": 8}[kind[6]]
        H, W = (64, 64) if kind.endswith("s") else (256, 256)
    x, w, bias = c.rand(91, N, H, W, cinp), c.rand(92, cout, cinp, 3, 3, scale=0.2), c.rand(93, cout)
    packed = c.zeros(c.lib.bbdm_conv_packed_floats(cout, cinp, 3))
    c.call("bbdm_conv_pack_weight_f32", P(w), P(packed), cout, cinp, cinp, 3, c.st)
    sc, bi = (c.rand(94, N, cinp), c.rand(95, N, cinp)) if pre else (None, None)
    out = c.zeros(N * H * W * cout)
    G = 32
    st = c.zeros(c.lib.bbdm_groupnorm_stats_bytes(N, G) // 8, c.torch.int64) if stats else None
    c.call("bbdm_conv2d_nhwc_stats_f32", P(x), cinp, P(packed), P(bias), None, 0, P(out), cout, 0, None, 0, P(sc), P(bi), cinp if pre else 0,
           1 if pre else 0, N, H, W, cinp, cout, 3, P(st), cout // G if stats else 0, 0, None, 0, 0, c.st)
    return [out] + ([st] if stats else [])


def linear_bwd_case(c, N, In, Out):
    dy, x, w = c.rand(101, N, Out), c.rand(102, N, In), c.rand(103, Out, In, scale=0.1)
    dx, dw, db = c.zeros(N * In), c.zeros(Out * In), c.zeros(Out)
    ws = c.zeros(max(1, c.lib.bbdm_linear_bwd_workspace_floats(N, In, Out)))
    c.call("bbdm_linear_bwd_f32", P(dy), P(x), P(w), P(dx), P(dw), P(db), P(ws), N, In, Out, 1, c.st)
    return [dx, dw, db]


def conv1x1_q_case(c, h2, res, cout):
    """The wide 1x1 layers on the pipelined kernel with an fp32 A operand: 256-column tiles where Cout fills them, with / without residual."""
    pix, cin = 300, 64
    x, w, bias = c.rand(111, pix, cin), c.rand(112, cout, cin, scale=0.1), c.rand(113, cout)
    r = c.rand(114, pix, cout) if res else None
    pf = c.zeros(c.lib.bbdm_conv_packed_floats(cout, cin, 1))
    c.call("bbdm_conv_pack_weight_f32", P(w), P(pf), cout, cin, cin, 1, c.st)
    out, bound = c.zeros(pix * cout), c.scalar(8.0)
    if h2:
        b = c.bytes_(c.lib.bbdm_gemm_h2p_b_bytes(1, cin, cout))
        c.call("bbdm_gemm_h2p_pack_b_f32", P(pf), P(b), P(bound), 1.0, 1, cin, cout, c.st)
        c.call("bbdm_conv1x1_h2q_f32", P(x), cin, P(b), P(bias), P(r), cout, P(out), cout, pix, cin, cout, P(bound), P(bound), c.st)
    else:
        b = c.bytes_(c.lib.bbdm_gemm_bf3p_b_bytes(1, cin, cout))
        c.call("bbdm_gemm_bf3p_pack_b_f32", P(pf), P(b), 1, cin, cout, c.st)
        c.call("bbdm_conv1x1_bf3q_f32", P(x), cin, P(b), P(bias), P(r), cout, P(out), cout, pix, cin, cout, c.st)
    return [out]


def conv1x1_bf3_case(c, res, batch8):
    """gemm_bf3_kernel: with / without residual (the 1x1 entry), and a batch of 8 (one entry per XCD) through bbdm_gemm_bf3_f32."""
    T, cin, cout = 256, 32, 40
    batch = 8 if batch8 else 1
    x, w = c.rand(121, batch * T, cin), c.rand(122, batch, cin // 16 * 128 * 16, scale=0.1)
    pk = c.zeros(c.lib.bbdm_gemm_bf3_packed_halfs(batch, cin, cout), c.torch.int16)
    c.call("bbdm_gemm_bf3_pack_f32", P(w), P(pk), batch, cin, cout, c.st)
    out = c.zeros(batch * T * cout)
    if batch8:
        c.call("bbdm_gemm_bf3_f32", P(x), P(pk), P(out), batch, T, cin, cout, c.st)
    else:
        bias, r = c.rand(123, cout), (c.rand(124, T, cout) if res else None)
        c.call("bbdm_conv1x1_bf3_f32", P(x), cin, P(pk), P(bias), P(r), cout, P(out), cout, T, cin, cout, c.st)
    return [out]


def conv_wgrad_case(c, ks, cin, cout):
    N, H, W = 2, 12, 12
    x, dy = c.rand(131, N, H, W, cin), c.rand(132, N, H, W, cout)
    ws = c.zeros(max(1, c.lib.bbdm_conv_wgrad_workspace_floats(N, H, W, cin, cout, ks)))
    dw, db = c.zeros(cout * cin * ks * ks), c.zeros(cout)
    c.call("bbdm_conv_wgrad_f32", P(x), cin, P(dy), cout, P(dw), P(db), P(ws), ws.numel(), N, H, W, cin, cout, ks, c.st)
    return [dw, db]


def winograd_wgrad_case(c, m, planes, cin, cout, bias):
    """The weight gradient in the Winograd domain: fp32 stages (dY transform, TN GEMM on 256- or 128-row tiles, finish) or the bf16
    planes (input transform with the transposed copy, dY planes, bbdm_gemm_bf3p_tn_f32, finish with / without the bias sums)."""
    N, H = 2, hw_of(m, True)
    W = H
    x, dy = c.rand(141, N, H, W, cin), c.rand(142, N, H, W, cout)
    dw, db = c.zeros(cout * cin * 9), c.zeros(cout)
    if not planes:
        ws = c.zeros(c.lib.bbdm_winograd_wgrad_workspace_floats(m, N, H, W, cin, cout))
        c.call("bbdm_conv3x3_winograd_wgrad_f32", m, P(x), cin, P(dy), cout, P(dw), P(db) if bias else None, P(ws), N, H, W, cin, cout, c.st)
        return [dw, db]
    pl, Tp = planes_of(m), c.lib.bbdm_winograd_tiles(m, N, H, W)
    T = N * -(-H // m) * -(-W // m)
    Vp, Vt = c.bytes_(c.lib.bbdm_gemm_bf3p_a_bytes(pl, Tp, cin)), c.bytes_(c.lib.bbdm_gemm_bf3p_tn_at_bytes(pl, Tp, cin))
    dMt, dm11 = c.bytes_(c.lib.bbdm_gemm_bf3p_tn_bt_bytes(pl, Tp, cout)), c.zeros(Tp * cout)
    c.call("bbdm_winograd_input_bf3p_tr_f32", m, P(x), cin, P(Vp), None, None, 0, 0, 0, N, H, W, cin, P(Vt), c.st)
    c.call("bbdm_winograd_dy_transform_bf3p_f32", m, P(dy), cout, P(dMt), P(dm11), N, H, W, cout, c.st)
    if not c.lib.bbdm_gemm_bf3p_tn_supported(Tp, cin, cout):
        raise Rejected("gemm_bf3p_tn: unsupported shape")
    splits = c.lib.bbdm_gemm_bf3p_tn_splits(pl, Tp, cin, cout)
    dU = c.zeros(splits * pl * cin * cout)
    c.call("bbdm_gemm_bf3p_tn_f32", P(Vt), P(dMt), P(dU), pl, Tp, cin, cout, c.st)
    if bias:
        c.call("bbdm_winograd_wgrad_finish_bias_f32", m, P(dU), splits, P(dw), cin, cout, P(dm11), T, P(db), c.st)
    else:
        c.call("bbdm_winograd_wgrad_finish_f32", m, P(dU), splits, P(dw), cin, cout, c.st)
    return [dU, dw, db]


def linear_case(c, N, In, Out, packed):
    """bbdm_linear_f32: the MFMA kernel from 2048 outputs (one or two 32-row blocks), else the thread kernel, vector loads or not, under
    and over 64 KB of staging; bbdm_linear_packed_f32 on packed weights."""
    x, w, b = c.rand(151, N, In), c.rand(152, Out, In, scale=0.1), c.rand(153, Out)
    y = c.zeros(N * Out)
    if packed:
        if not c.lib.bbdm_linear_packed_supported(N, In, Out):
            raise Rejected("linear_packed: unsupported shape")
        wp = c.bytes_(c.lib.bbdm_linear_packed_bytes(Out, In))
        c.call("bbdm_linear_pack_f32", P(w), P(wp), Out, In, c.st)
        c.call("bbdm_linear_packed_f32", P(x), P(wp), P(b), P(y), N, In, Out, 1, 0, c.st)
    else:
        c.call("bbdm_linear_f32", P(x), P(w), P(b), P(y), N, In, Out, 1, 0, c.st)
    return [y]


# ---- the elementwise files (bridge.hip, optim.hip, loss_meter.hip): every entry point, at the smallest shapes that reach each route --------
def ints(c, vals):
    return c.torch.tensor(vals, dtype=c.torch.int64).to(c.dev)


def floats(c, vals):
    return c.torch.tensor(vals, dtype=c.torch.float32).to(c.dev)


def rand_off(c, seed, n, off, scale=1.0):
    """n seeded floats that start `off` floats past an allocation (off = 1: no pointer is 16-byte aligned)."""
    return c.rand(seed, n + off, scale=scale)[off:]


def zeros_off(c, n, off):
    return c.zeros(n + off)[off:]


def per_image(c, vals, N):
    """An int64 value per image: `vals` repeated to N entries."""
    return ints(c, (vals * (N // len(vals) + 1))[:N])


def schedule(c, T=10):
    """m_t rising from 0.001 to 0.999 and the bridge's variance 2 (m - m^2), as BrownianBridgeModel.register_schedule forms them."""
    m = c.torch.linspace(0.001, 0.999, T, dtype=c.torch.float32)
    return m.to(c.dev), (2.0 * (m - m * m)).to(c.dev)


# (per_sample, offset): a ragged last group; two blocks in x on 16-byte accesses; the same on element accesses with every group full
IMAGE_SHAPES = {"tail": (7, 0), "vec": (1032, 0), "elem": (1032, 1)}


def p_step_image_case(c, form, shape, objective, clip, alias, N=3):
    """The four per-image step entries.  States 0, 1, 2 over the three images; the request forms carry clip in bit 2 and eta per image."""
    ps, off = IMAGE_SHAPES.get(shape, (shape, 0))
    requests, philox = "requests" in form, "philox" in form
    n = max(N * ps, 1)                                    # (per_sample = 0 is refused before any access; no pointer may be null)
    x_t, y, pred = rand_off(c, 201, n, off), rand_off(c, 202, n, off), rand_off(c, 203, n, off)
    m_tab, var_tab = schedule(c)
    t, t_next = per_image(c, [7, 4, 1], N), per_image(c, [5, 2, 0], N)
    flag = per_image(c, [4, 5, 2] if requests and clip else [0, 1, 2], N)
    x_next, x0 = zeros_off(c, n, off), zeros_off(c, n, off)
    al = zeros_off(c, n, off) if alias else None
    src = (per_image(c, [11, 12, 13], N), per_image(c, [0, 5, 2 ** 33], N)) if philox else (rand_off(c, 204, n, off),)
    eta = floats(c, ([1.0, 0.5, 0.25] * (N // 3 + 1))[:N])
    par = (P(eta),) if requests else (0.75, clip)
    name = {"batched": "bbdm_bb_p_sample_step_batched_f32", "requests": "bbdm_bb_p_sample_step_requests_f32",
            "philox": "bbdm_bb_p_sample_step_philox_f32", "requests_philox": "bbdm_bb_p_sample_step_requests_philox_f32"}[form]
    c.call(name, P(x_t), P(y), P(pred), *map(P, src), P(m_tab), P(var_tab), P(t), P(t_next), P(flag), *par, objective, P(x_next), P(x0), P(al),
           N, ps, c.st)
    return [x_next, x0] + ([al] if alias else [])


def q_sample_philox_case(c, shape, objective, N=3):
    ps, off = IMAGE_SHAPES.get(shape, (shape, 0))
    n = max(N * ps, 1)
    x0, y = rand_off(c, 211, n, off), rand_off(c, 212, n, off)
    m_tab, var_tab = schedule(c)
    x_t, target = zeros_off(c, n, off), zeros_off(c, n, off)
    seed, ordinal, t = per_image(c, [11, 12, 13], N), per_image(c, [0, 5, 2 ** 33], N), per_image(c, [7, 4, 1], N)
    c.call("bbdm_bb_q_sample_philox_f32", P(x0), P(y), P(seed), P(ordinal), P(t), P(m_tab), P(var_tab), P(x_t), P(target), N, ps, objective, c.st)
    return [x_t, target]


def q_sample_cached_case(c, shape, philox, stats, objective, bad, N=3):
    """Rows gathered from a cache of M = 4; hw = per_sample / 3 for 1032 (three channels), 7 for 7; `bad`: one index = M (NaN fill)."""
    ps, off = IMAGE_SHAPES.get(shape, (shape, 0))
    M, hw = 4, (344 if ps == 1032 else max(ps, 1))
    n = max(N * ps, 1)
    C = max(ps // hw, 1)
    ori, cond = rand_off(c, 221, M * max(ps, 1), off), rand_off(c, 222, M * max(ps, 1), off)
    idx_ori, idx_cond = per_image(c, [2, M if bad else 0, 3], N), per_image(c, [1, 3, 0], N)
    st = [c.rand(223, C), c.rand(224, C).abs() + 0.5, c.rand(225, C), c.rand(226, C).abs() + 0.5] if stats else [None] * 4
    seed, ordinal, t = per_image(c, [11, 12, 13], N), per_image(c, [0, 5, 2 ** 33], N), per_image(c, [7, 4, 1], N)
    noise = None if philox else rand_off(c, 227, n, off)
    m_tab, var_tab = schedule(c)
    x_t, target, y_out = zeros_off(c, n, off), zeros_off(c, n, off), zeros_off(c, n, off)
    head = (P(ori), P(cond), M, P(idx_ori), P(idx_cond), *map(P, st), hw)
    tail = (P(t), P(m_tab), P(var_tab), P(x_t), P(target), P(y_out), N, ps, objective, c.st)
    if philox:
        c.call("bbdm_bb_q_sample_cached_philox_f32", *head, P(seed), P(ordinal), *tail)
    else:
        c.call("bbdm_bb_q_sample_cached_f32", *head, P(noise), *tail)
    return [x_t, target, y_out]


def philox_normal_case(c, shape, domain, N=3):
    ps, off = IMAGE_SHAPES.get(shape, (shape, 0))
    out = zeros_off(c, max(N * ps, 1), off)
    seed, ordinal = per_image(c, [11, 12, 13], N), per_image(c, [0, 5, 2 ** 33], N)
    c.call("bbdm_philox_normal_f32", P(out), P(seed), P(ordinal), domain, N, ps, c.st)
    return [out]


def p_step_scalar_case(c, is_last, clip, objective, alias):
    N, ps = 3, 7
    n = N * ps
    x_t, y, pred, noise = c.rand(231, n), c.rand(232, n), c.rand(233, n), c.rand(234, n)
    m_tab, var_tab = schedule(c)
    x_next, x0, al = c.zeros(n), c.zeros(n), (c.zeros(n) if alias else None)
    c.call("bbdm_bb_p_sample_step_f32", P(x_t), P(y), P(pred), P(noise), P(m_tab), P(var_tab), 7, 5, is_last, 0.75, clip, objective,
           P(x_next), P(x0), P(al), N, ps, c.st)
    return [x_next, x0] + ([al] if alias else [])


def q_sample_scalar_case(c, which, objective):
    N, ps = 3, 7
    n = N * ps
    a, b, e = c.rand(241, n), c.rand(242, n), c.rand(243, n)
    m_tab, var_tab = schedule(c)
    t = ints(c, [7, 4, 1])
    if which == "q_sample":
        x_t, target = c.zeros(n), c.zeros(n)
        c.call("bbdm_bb_q_sample_f32", P(a), P(b), P(e), P(t), P(m_tab), P(var_tab), P(x_t), P(target), N, ps, objective, c.st)
        return [x_t, target]
    x0 = c.zeros(n)
    c.call("bbdm_bb_predict_x0_f32", P(a), P(b), P(e), P(t), P(m_tab), P(var_tab), P(x0), N, ps, objective, c.st)
    return [x0]


def loss_case(c, bwd, count, loss_type):
    a, b = c.rand(251, count), c.rand(252, count)
    if bwd:
        dpred = c.zeros(count)
        gscale = c.scalar(0.5)
        c.call("bbdm_bb_loss_bwd_f32", P(a), P(b), P(gscale), P(dpred), count, loss_type, c.st)
        return [dpred]
    cell, out = c.zeros(4, c.torch.int64), c.zeros(1)
    c.call("bbdm_bb_loss_f32", P(a), P(b), P(cell), P(out), count, loss_type, c.st)
    return [cell, out]


def layout_case(c, to_nhwc, Cb):
    N, H, W, Ca, Cpad, ld = 2, 3, 5, 3, 4, 4
    if to_nhwc:
        a, b = c.rand(261, N * Ca * H * W), (c.rand(262, N * Cb * H * W) if Cb else None)
        out = c.zeros(N * H * W * ld)
        c.call("bbdm_nchw_to_nhwc_f32", P(a), Ca, P(b), Cb, P(out), ld, Cpad, N, H, W, c.st)
    else:
        x, out = c.rand(263, N * H * W * ld), c.zeros(N * Ca * H * W)
        c.call("bbdm_nhwc_to_nchw_f32", P(x), ld, P(out), N, H, W, Ca, c.st)
    return [out]


def philox_raw_case(c, n):
    g = c.torch.Generator().manual_seed(271)
    ck = c.torch.randint(-2 ** 31, 2 ** 31, (n, 6), generator=g, dtype=c.torch.int64).to(c.torch.int32).to(c.dev)
    out = c.zeros(4 * n, c.torch.int32)
    c.call("bbdm_philox_raw_u32", P(ck), P(out), n, c.st)
    return [out]


def latent_stats_case(c, hw, row_blocks):
    M, C = 5, 3
    z = c.rand(281, M * C * hw)
    cells = c.zeros(2 * C * 4, c.torch.int64)
    mean, var, stdev = c.zeros(C), c.zeros(C), c.zeros(C)
    c.call("bbdm_latent_channel_stats_f32", P(z), M, C, hw, P(cells), P(mean), P(var), P(stdev), row_blocks, c.st)
    return [cells, mean, var, stdev]


def opt_table(c, mom, sq, nan=False):
    """-> (device table, chunks, every buffer).  Rows as bbdm_amd.optim._ChunkTable lays them out: 16 390 elements with every pointer
    aligned (a full chunk and a tail chunk), 16 390 one float past an alignment, 3 without a gradient, 16 384 without a shadow."""
    ce = c.lib.bbdm_opt_chunk_elems()
    rows, bufs = [], []
    for i, (n, off, has_g, has_s) in enumerate(((16390, 0, 1, 1), (16390, 1, 1, 1), (3, 0, 0, 1), (16384, 0, 1, 0))):
        p = rand_off(c, 300 + 10 * i, n, off)
        g = rand_off(c, 301 + 10 * i, n, off, scale=0.1) if has_g else None
        m = rand_off(c, 302 + 10 * i, n, off, scale=0.1) if mom else None
        v = rand_off(c, 303 + 10 * i, n, off, scale=0.1).abs() if sq else None
        s = rand_off(c, 304 + 10 * i, n, off) if has_s else None
        if nan and i == 0:
            g[5] = float("nan")
        rows.append((p, g, m, v, s))
        bufs += [x for x in (p, g, m, v, s) if x is not None]
    ent = []
    for p, g, m, v, s in rows:
        for o in range(0, p.numel(), ce):
            ent.append([0 if x is None else x.data_ptr() + 4 * o for x in (p, g, m, v, s)] + [min(ce, p.numel() - o)])
    return c.torch.tensor(ent, dtype=c.torch.int64).to(c.dev), len(ent), bufs


def arg(v):
    return v.data_ptr() if hasattr(v, "data_ptr") else v


def clip_args(c, clip):
    """plain: the entry without a clip buffer; "coef": {norm, coef < 1, ok}; "skip": a non-finite norm under skip_nonfinite."""
    if clip == "plain":
        return "_f32", ()
    buf = floats(c, [2.0, 0.5, 1.0, 0.0] if clip == "coef" else [float("nan"), float("nan"), 0.0, 0.0])
    return "_clip_f32", (buf, 1 if clip == "skip" else 0)


def adam_case(c, do_adam, wd, ema_mode, step, clip):
    table, n, bufs = opt_table(c, True, True)
    sfx, extra = clip_args(c, clip)
    c.call("bbdm_adam_ema_step" + sfx, P(table), n, do_adam, 1e-3, 0.9, 0.999, 1e-8, wd, step, ema_mode, 0.999, *map(arg, extra), c.st)
    return bufs


def sgd_case(c, momentum, nesterov, first, dampening, clip):
    table, n, bufs = opt_table(c, momentum != 0, False)
    sfx, extra = clip_args(c, clip)
    c.call("bbdm_sgd_ema_step" + sfx, P(table), n, 1e-2, momentum, dampening, 0.01, nesterov, first, 1, 0.999, *map(arg, extra), c.st)
    return bufs


def rmsprop_case(c, momentum, ema_mode, clip):
    table, n, bufs = opt_table(c, momentum != 0, True)
    sfx, extra = clip_args(c, clip)
    c.call("bbdm_rmsprop_ema_step" + sfx, P(table), n, 1e-2, 0.99, 1e-8, 0.01, momentum, ema_mode, 0.999, *map(arg, extra), c.st)
    return bufs


def grad_norm_case(c, max_norm, nan, scale):
    table, n, bufs = opt_table(c, False, False, nan=nan)
    cells = c.zeros(c.lib.bbdm_grad_norm_cells_bytes() // 8, c.torch.int64)
    out, skipped = c.zeros(4), c.zeros(1, c.torch.int64)
    c.call("bbdm_grad_sqnorm_f32", P(table), n, P(cells), c.st)
    c.call("bbdm_grad_norm_finalize_f32", P(cells), max_norm, P(out), P(skipped), c.st)
    if scale:
        c.call("bbdm_grad_scale_f32", P(table), n, P(out), c.st)
    return [cells, out, skipped] + bufs


def loss_meter_case(c, per_sample, off, loss_type, want_image, stage):
    """stage "per_image"; "accumulate": + a t vector with one negative value and one >= T; "read": + the table read back."""
    N, T, B = 3, 10, 4
    a, b = rand_off(c, 401, N * per_sample, off), rand_off(c, 402, N * per_sample, off)
    cells = c.zeros(N * 4, c.torch.int64)
    per_image = c.zeros(N) if want_image else None
    c.call("bbdm_loss_meter_per_image_f32", P(a), P(b), P(cells), P(per_image), N, per_sample, loss_type, c.st)
    outs = [cells] + ([per_image] if want_image else [])
    if stage == "per_image":
        return outs
    meter, counts = c.zeros(2 * B * 4, c.torch.int64), c.zeros(B + 1, c.torch.int64)
    t = ints(c, [-1, 5, 12])
    c.call("bbdm_loss_meter_accumulate", P(cells), P(t), P(meter), P(counts), N, per_sample, T, B, c.st)
    outs += [meter, counts]
    if stage == "read":
        s, sq = c.zeros(B, c.torch.float64), c.zeros(B, c.torch.float64)
        c.call("bbdm_loss_meter_read", P(meter), P(s), P(sq), B, c.st)
        outs += [s, sq]
    return outs


def elementwise_grid():
    prod = itertools.product
    forms = ("batched", "requests", "philox", "requests_philox")
    for form, shape, objective, clip, alias in prod(forms, IMAGE_SHAPES, (0, 1, 2), (0, 1), (0, 1)):
        yield "p_step_image", dict(form=form, shape=shape, objective=objective, clip=clip, alias=alias), p_step_image_case
    for shape, objective in prod(IMAGE_SHAPES, (0, 1, 2)):
        yield "q_sample_philox", dict(shape=shape, objective=objective), q_sample_philox_case
    for shape, philox, stats, objective, bad in prod(IMAGE_SHAPES, (0, 1), (0, 1), (0, 1, 2), (0, 1)):
        yield "q_sample_cached", dict(shape=shape, philox=philox, stats=stats, objective=objective, bad=bad), q_sample_cached_case
    for shape, domain in prod(IMAGE_SHAPES, (0, 1)):
        yield "philox_normal", dict(shape=shape, domain=domain), philox_normal_case
    for is_last, clip, objective, alias in prod((0, 1), (0, 1), (0, 1, 2), (0, 1)):
        yield "p_step_scalar", dict(is_last=is_last, clip=clip, objective=objective, alias=alias), p_step_scalar_case
    for which, objective in prod(("q_sample", "predict_x0"), (0, 1, 2)):
        yield "q_sample_scalar", dict(which=which, objective=objective), q_sample_scalar_case
    for bwd, count, loss_type in prod((0, 1), (7, 5000), (0, 1)):
        yield "loss", dict(bwd=bwd, count=count, loss_type=loss_type), loss_case
    for to_nhwc, Cb in ((1, 1), (1, 0), (0, 0)):
        yield "layout", dict(to_nhwc=to_nhwc, Cb=Cb), layout_case
    yield "philox_raw", dict(n=5), philox_raw_case
    for hw, row_blocks in prod((8, 7), (0, 2)):
        yield "latent_stats", dict(hw=hw, row_blocks=row_blocks), latent_stats_case
    for do_adam, wd, ema_mode, step, clip in prod((0, 1), (0.0, 0.01), (0, 1, 2), (1, 7), ("plain", "coef", "skip")):
        yield "adam", dict(do_adam=do_adam, wd=wd, ema_mode=ema_mode, step=step, clip=clip), adam_case
    for momentum, nesterov, first, dampening, clip in prod((0.0, 0.9), (0, 1), (0, 1), (0.0, 0.1), ("plain", "coef")):
        yield "sgd", dict(momentum=momentum, nesterov=nesterov, first=first, dampening=dampening, clip=clip), sgd_case
    for momentum, ema_mode, clip in prod((0.0, 0.9), (0, 1, 2), ("plain", "coef", "skip")):
        yield "rmsprop", dict(momentum=momentum, ema_mode=ema_mode, clip=clip), rmsprop_case
    for max_norm, nan in prod((float("inf"), 0.5), (0, 1)):
        yield "grad_norm", dict(max_norm=max_norm, nan=nan, scale=0), grad_norm_case
    yield "grad_norm", dict(max_norm=0.5, nan=0, scale=1), grad_norm_case
    for per_sample, off, loss_type, want_image in prod((7, 2052), (0, 1), (0, 1), (0, 1)):
        yield "loss_meter", dict(per_sample=per_sample, off=off, loss_type=loss_type, want_image=want_image, stage="per_image"), loss_meter_case
    for stage in ("accumulate", "read"):
        yield "loss_meter", dict(per_sample=7, off=0, loss_type=1, want_image=0, stage=stage), loss_meter_case
    # refusals: the error text must match too
    for N, shape in ((65536, 1), (3, 0)):
        for form in forms:
            yield "p_step_image", dict(form=form, shape=shape, objective=0, clip=0, alias=0, N=N), p_step_image_case
        yield "q_sample_philox", dict(shape=shape, objective=0, N=N), q_sample_philox_case
        for philox in (0, 1):
            yield "q_sample_cached", dict(shape=shape, philox=philox, stats=0, objective=0, bad=0, N=N), q_sample_cached_case
        yield "philox_normal", dict(shape=shape, domain=0, N=N), philox_normal_case
    yield "adam", dict(do_adam=1, wd=0.0, ema_mode=3, step=1, clip="plain"), adam_case
    yield "rmsprop", dict(momentum=0.0, ema_mode=3, clip="plain"), rmsprop_case


def grid():
    prod = itertools.product
    for m, pre, up, form, idx64 in prod((2, 4, 6, 7, 8), (0, 1), (0, 1), INPUT_FORMS, (0, 1)):
        for ragged in ((0, 1) if m >= 6 and m != 7 and idx64 == 0 and not up else (0,)):
            yield "winograd_input", dict(m=m, pre=pre, up=up, form=form, idx64=idx64, ragged=ragged), input_case
    for m, cout, res, nstats, splits in prod((2, 4, 6, 7, 8), (40, 128), ("none", "image", "up"), (0, 1, 2), (1, 2)):
        if splits == 2 and m >= 6:
            continue
        phases = 1 if m == 7 else 0
        for shape, cpg in (("two", 8), ("one", 8)) + ((("ragged", 4),) if m in (6, 8) else ()):
            yield "winograd_output", dict(m=m, cout=cout, res=res, nstats=nstats, cpg=cpg, splits=splits, phases=phases, shape=shape), output_case
    for m in (2, 4):                                      # the phase form on the ordinary tiles
        yield "winograd_output", dict(m=m, cout=128, res="none", nstats=1, cpg=8, splits=1, phases=1, shape="two"), output_case
    # enough workgroups for the narrow-group rule to keep more than two tiles per workgroup
    yield "winograd_output", dict(m=2, cout=256, res="none", nstats=1, cpg=8, splits=1, phases=0, shape="wide"), output_case
    for m, dgrad, form in prod((2, 4, 6, 7, 8), (0, 1), ("f32", "bf3p", "h2p")):
        yield "winograd_pack", dict(m=m, dgrad=dgrad, form=form), pack_case
    for m, h2 in prod((2, 4, 6, 8), (0, 1)):
        yield "winograd_dy", dict(m=m, h2=h2), dy_case
    for m, which in prod((2, 4, 6, 7, 8), range(5)):
        yield "transform_1d", dict(m=m, which=which), transform_1d_case
    for ch, bf3, pipe, new_order in prod((16, 32, 64, 128), (0, 1, 2), (0, 1, 3), (0, 1)):
        yield "attention", dict(ch=ch, bf3=bf3, pipe=pipe, new_order=new_order, form="fwd", T=160), attention_case
    for ch, bf3 in prod((16, 32, 64, 128), (0, 1, 2)):
        yield "attention", dict(ch=ch, bf3=bf3, pipe=1, new_order=0, form="cross", T=160), attention_case
    for ch, new_order, form in prod((16, 32, 64, 128), (0, 1), ("planes", "planes_h2")):
        yield "attention", dict(ch=ch, bf3=1, pipe=3, new_order=new_order, form=form, T=128), attention_case
    for ch, new_order in prod((16, 32, 64, 128), (0, 1)):
        yield "attention_bwd", dict(ch=ch, new_order=new_order), attention_bwd_case
    for e_dim in range(1, 9):
        yield "vq_nearest", dict(e_dim=e_dim), vq_case
    for variant, np_, res, cout in prod((4, 5, 7, 6), (2, 3), (0, 1), (40, 256)):
        yield "tile_gemm", dict(variant=variant, np_=np_, res=res, cout=cout, T=256), tile_gemm_case
    for h2, res in prod((0, 1), (0, 1)):
        yield "conv1x1_small", dict(h2=h2, res=res), small_1x1_case
    for kind, stats in prod(("stem8", "stem4"), (0, 1)):
        yield "conv2d", dict(kind=kind, stats=stats, pre=0), conv_case
    for kind, pre in prod(("narrow3s", "narrow4s", "narrow8s", "narrow3l", "narrow8l"), (0, 1)):
        yield "conv2d", dict(kind=kind, stats=0, pre=pre), conv_case
    yield "linear_bwd", dict(N=40, In=512, Out=96), linear_bwd_case            # 80 KB of staging: above the default LDS limit
    yield "linear_bwd", dict(N=8, In=64, Out=40), linear_bwd_case
    # ---- launchers beyond the issue's list that the same refactor rewrote
    for m in (6, 8):                                      # BBDM_CONV_OUT_PHASES on the large tiles
        yield "winograd_output", dict(m=m, cout=128, res="none", nstats=1, cpg=8, splits=1, phases=1, shape="two"), output_case
    for pre in (0, 1):
        yield "conv2d", dict(kind="narrow4l", stats=0, pre=pre), conv_case
    # eight chunks per workgroup and few workgroups: the three-stage ring of the 128 x 128 tile
    for np_, res in prod((2, 3), (0, 1)):
        yield "tile_gemm", dict(variant=7, np_=np_, res=res, cout=40, T=256, cin=128), tile_gemm_case
    for h2, res, cout in prod((0, 1), (0, 1), (40, 256)):
        yield "conv1x1_q", dict(h2=h2, res=res, cout=cout), conv1x1_q_case
    for res, batch8 in ((0, 0), (1, 0), (0, 1)):
        yield "conv1x1_bf3", dict(res=res, batch8=batch8), conv1x1_bf3_case
    for ks, cin, cout in prod((1, 3), (32, 128), (40,)):
        yield "conv_wgrad", dict(ks=ks, cin=cin, cout=cout), conv_wgrad_case
    for m, cin in prod((2, 4, 6), (32, 256)):
        yield "winograd_wgrad", dict(m=m, planes=0, cin=cin, cout=40, bias=1), winograd_wgrad_case
    for m, bias in prod((2, 4, 6, 8), (0, 1)):
        yield "winograd_wgrad", dict(m=m, planes=1, cin=32, cout=40, bias=bias), winograd_wgrad_case
    yield "winograd_wgrad", dict(m=4, planes=1, cin=32, cout=256, bias=1), winograd_wgrad_case
    for N, In, Out in ((8, 64, 2048), (40, 64, 2048), (40, 512, 2048), (8, 64, 40), (8, 63, 40), (40, 512, 40)):
        yield "linear", dict(N=N, In=In, Out=Out, packed=0), linear_case
    for N, In in ((8, 64), (32, 512)):
        yield "linear", dict(N=N, In=In, Out=96, packed=1), linear_case
    yield from elementwise_grid()


def child(path, emu, out_path):
    sys.path.insert(0, ROOT)
    import torch
    from bbdm_amd import _lib
    lib = _lib.bind(path) if emu else _lib.load()
    if not emu:
        assert os.path.samefile(_lib.LIB_PATH, path), (_lib.LIB_PATH, path)
    c = Ctx(lib, "cpu" if emu else "cuda")
    rows = []
    for name, args, fn in grid():
        # only a refusal by the library is a result; anything else (a GPU fault surfacing in synchronize() or in the copy to the
        # host, an error in this tool) ends the child at once, and with it the whole comparison
        try:
            outs = fn(c, **args)
        except Rejected as e:
            outs, hashes = None, ["error: " + str(e)]
        if not emu:
            torch.cuda.synchronize()
        if outs is not None:
            hashes = [hashlib.sha256(o.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for o in outs]
        rows.append({"call": name, "args": args, "sha256": hashes})
    with open(out_path, "w") as f:
        json.dump(rows, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--emu", action="store_true", help="both libraries are tools/hipemu builds (CPU)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(os.path.abspath(a.old), a.emu, a.child)
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, path in enumerate((a.old, a.new)):
            path = os.path.abspath(path)
            out = os.path.join(tmp, f"{i}.json")
            env = dict(os.environ)
            if not a.emu:
                env["BBDM_HIP_LIB"] = path
            cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), path, path, "--child", out]
            rc = subprocess.call(cmd + (["--emu"] if a.emu else []), env=env)
            if rc != 0:
                print(f"lib_ab: the run of {path} failed (exit status {rc}); nothing more is started")
                return 2
            results.append(json.load(open(out)))
    old, new = results
    errors = sum(1 for r in old if r["sha256"][0].startswith("error"))
    for ro, rn in zip(old, new):
        if ro != rn:
            print(f"lib_ab: DIFFERENT at {ro['call']} {json.dumps(ro['args'])}\n  old: {ro['sha256']}\n  new: {rn['sha256']}")
            return 1
    if len(old) != len(new):
        print(f"lib_ab: {len(old)} calls against {len(new)}")
        return 1
    print(f"lib_ab: {len(old)} calls ({errors} rejected alike by both), {sum(len(r['sha256']) for r in old)} buffers: zero differences")
    return 0


if __name__ == "__main__":
    sys.exit(main())
