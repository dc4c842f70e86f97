"""Shared bodies of the kernel-level tests of the VQGAN first stage's own entry points (csrc/firststage.hip, the batched activation GEMM
of csrc/conv_igemm.hip, the decimating modes of bbdm_groupnorm_apply_f32): bbdm_gemm_pack_b_f32 / bbdm_gemm_batched_f32 /
bbdm_gemm_packed_b_floats, bbdm_softmax_rows_f32, bbdm_groupnorm_apply_f32 with resample 3 and 4, bbdm_vq_nearest_f32 at every
instantiated e_dim and at pitches wider than e_dim.

Every function takes the device the tensors live on (a GPU, or the CPU under tests/emu_backend.emulated_backend()) and is driven by
tests/test_first_stage_kernels_gpu.py and tests/test_first_stage_kernels_emu_cpu.py.  Every reference is fp64 on the CPU and every
tolerance is derived from the number format (u = 2^-24, the unit roundoff of fp32), not from what the kernels give; each test prints
the worst observed ratio to its tolerance before it asserts."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_ops as ops
from fixtures import rel_err

U = 2.0 ** -24
NAN = float("nan")
SENT = -7.25            # sentinel of destination padding: exactly representable, never a result
TOL = 2e-5              # tests/test_kernels_gpu.py: fp32 with another summation order, relative to the output's largest magnitude


def _untouched(t: torch.Tensor) -> bool:
    return bool((t == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# a. batched activation GEMM
# ---------------------------------------------------------------------------------------------------------------------------------
GEMM_CASES = [
    # batch, rows, K, R, transposed
    (2, 36, 36, 36, 0),         # rows % 32 != 0: image of width 1; rows < 256; 4 valid floats in the last K chunk
    (2, 36, 36, 20, 1),
    (1, 300, 20, 132, 0),       # width 1, two ragged 256-row tiles, two N tiles
    (3, 64, 132, 260, 1),       # width 32, three N tiles
    (1, 1056, 4, 36, 0),        # width 32, H = 33, one partial chunk
]
GEMM_PRODUCT_CASE = (2, 4096, 512, 4096, 0)      # the VQ-f4 AttnBlock's q k^T (first_stage_hip._attn), GPU only


def gemm_batched(dev, batch, rows, K, R, transposed):
    """out_b = A_b . B_b (B given [R x K] and used transposed, or given [K x R]) against fp64, element by element:

        |got - ref64|_ij <= K * 2^-23 * (|A| . |B|)_ij

    -- twice the classical worst-case bound K u / (1 - K u), u = 2^-24, of an fp32 dot product of length K summed in ANY order
    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), so it holds for every tiling / MFMA accumulation order.

    Operands as the plan may pass them: A with pitch K + 4 and one more row per batch element, pad columns and that row NaN (nothing
    outside [rows x K] may be read into the result); B with one NaN pad column; the packed buffer prefilled with NaN (the plan reuses
    ONE buffer for k and then v: a pack must overwrite everything the GEMM reads) with 16 guard floats behind it; out with pitch R + 3
    and one more row, prefilled with a sentinel.

    The check has teeth: the same comparison against an fp64 reference with the LAST k term dropped must fail for >= 99 % of the
    elements (a wrong last-chunk term cannot hide in the tolerance).  The tolerance grows as K^2 and one term does not, hence operands
    without entries near zero: every product is >= 1/16, the tolerance about 1.3e-7 K^2 (0.03 at K = 512)."""
    g = torch.Generator().manual_seed(1000 * rows + 10 * K + R + transposed)

    def operand(*shape):            # normal variates pushed away from zero: signs and sizes vary, no term is negligible
        x = torch.randn(*shape, generator=g)
        return torch.where(x < 0, x - 0.25, x + 0.25)
    A = operand(batch, rows, K)
    Bm = operand(batch, K, R) if transposed else operand(batch, R, K)
    a = torch.full((batch, rows + 1, K + 4), NAN)
    a[:, :rows, :K] = A
    b = torch.full((batch, Bm.shape[1], Bm.shape[2] + 1), NAN)
    b[:, :, :Bm.shape[2]] = Bm
    per = ops.gemm_packed_b_floats(R, K)
    assert per >= R * K
    packed = torch.full((batch * per + 16,), NAN).to(dev)
    out = torch.full((batch, rows + 1, R + 3), SENT).to(dev)
    ops.gemm_pack_b(b.to(dev), R, K, bool(transposed), packed=packed)
    ops.gemm_batched(a.to(dev), packed, rows, K, R, out=out)
    out, packed = out.cpu(), packed.cpu()

    got = out[:, :rows, :R].double()
    assert bool(torch.isfinite(got).all()), "NaN / inf in the result: padding was read"
    assert _untouched(out[:, :rows, R:]) and _untouched(out[:, rows:, :]), "wrote outside [rows x R]"
    assert bool(torch.isnan(packed[batch * per:]).all()), "pack wrote behind bbdm_gemm_packed_b_floats"
    assert bool(torch.isfinite(packed[:batch * per]).all()), "pack left part of its buffer unwritten"

    A64 = A.double()
    B64 = Bm.double() if transposed else Bm.double().transpose(1, 2)          # [batch, K, R]
    ref = A64 @ B64
    tol = K * 2.0 ** -23 * (A64.abs() @ B64.abs())
    ratio = float(((got - ref).abs() / tol).max())
    print(f"gemm_batched {(batch, rows, K, R, transposed)}: worst |err| / tolerance = {ratio:.3f}")
    assert ratio <= 1.0
    dropped = ref - A64[:, :, K - 1:K] * B64[:, K - 1:K, :]
    caught = float(((got - dropped).abs() > tol).double().mean())
    print(f"    against the reference without its last k term: {100 * caught:.2f} % of the elements exceed the tolerance")
    assert caught >= 0.99


# ---------------------------------------------------------------------------------------------------------------------------------
# b. row softmax
# ---------------------------------------------------------------------------------------------------------------------------------
SOFTMAX_CASES = [
    # rows, T, ld, max |scale * s|, scale
    (7, 36, 40, 3.0, 0.37),
    (5, 300, 300, 60.0, 0.37),
    (4, 64, 64, 1000.0, 0.37),
    (9, 4096, 4096, 20.0, 512 ** -0.5),       # the VQ-f4 AttnBlock: 4096 tokens, C^-1/2
]


def softmax_rows(dev, rows, T, ld, xm, scale):
    """In-place softmax(scale * s) over the first T columns of every row against fp64 softmax(float32(scale) * s).

    Elements whose exact value is >= 2^-100 (far above the fp32 subnormals): relative tolerance (8 Xm + T/64 + 32) u with u = 2^-24,
    Xm = max |scale * s| of the case:
      * the kernel rounds scale * s, the row maximum m of those, and their difference: an absolute error <= 4 u Xm in the argument of
        exp, i.e. that much relative error in every numerator and therefore in the denominator: 8 u Xm together;
      * expf within 2 ulp, in numerator and denominator: 8 u;
      * the denominator is a per-lane sum of T/64 non-negative terms and 6 shuffle steps: (T/64 + 6) u;
      * the remaining 18 u cover the reciprocal, the final multiply and the rounding of the stored value.
    Smaller elements must lie in [0, 2^-99].  Every row sums to 1 within (T/64 + 16) u: each of its T stored values is e_j / S rounded
    (2 u relative from the reciprocal and the multiply), S is the fp32 sum above.  The pad columns keep their sentinel.
    rows % 4 != 0 in three of the cases (4 rows per workgroup)."""
    g = torch.Generator().manual_seed(rows * 100000 + T)
    s0 = torch.randn(rows, T, generator=g)
    s0 = s0 * (xm / (scale * float(s0.abs().max())))
    s = torch.full((rows, ld), SENT)
    s[:, :T] = s0
    sc32 = torch.tensor(scale, dtype=torch.float32)
    arg = sc32.double() * s0.double()
    Xm = float(arg.abs().max())
    assert 0.9 * xm < Xm < 1.1 * xm
    ref = torch.softmax(arg, dim=1)
    got_full = ops.softmax_rows(s.to(dev), T, scale).cpu()
    got = got_full[:, :T].double()
    assert _untouched(got_full[:, T:])
    assert bool(torch.isfinite(got).all())
    big = ref >= 2.0 ** -100
    tol = (8 * Xm + T / 64 + 32) * U
    ratio = float(((got - ref).abs() / ref)[big].max()) / tol
    rowsum = float((got.sum(1) - 1).abs().max()) / ((T / 64 + 16) * U)
    print(f"softmax_rows {(rows, T, ld)} Xm = {Xm:.1f}: worst relative error / tolerance = {ratio:.3f}, "
          f"worst |row sum - 1| / tolerance = {rowsum:.3f}, {int((~big).sum())} elements below 2^-100")
    assert ratio <= 1.0
    small = got[~big]
    assert bool((small >= 0).all()) and bool((small <= 2.0 ** -99).all())
    assert rowsum <= 1.0


def softmax_uniform_row(dev):
    """A row whose elements all equal one large value (1e4): every exponent is exactly 0, the sum exactly T, the result 1 / T to 2 ulp
    (one rounding of the reciprocal, one of the product)."""
    for T, ld in ((36, 40), (300, 300), (64, 64), (4096, 4096)):
        s = torch.full((1, ld), SENT)
        s[:, :T] = 1e4
        got = ops.softmax_rows(s.to(dev), T, 0.37).cpu()
        assert _untouched(got[:, T:])
        ulp = 2.0 ** (math.floor(math.log2(1.0 / T)) - 23)
        err = float((got[:, :T].double() - 1.0 / T).abs().max())
        print(f"softmax_rows, uniform row of {T}: |got - 1/T| = {err / ulp:.2f} ulp")
        assert err <= 2 * ulp


# ---------------------------------------------------------------------------------------------------------------------------------
# c. decimation: bbdm_groupnorm_apply_f32 resample 3 (even positions) and 4 (odd positions)
# ---------------------------------------------------------------------------------------------------------------------------------
DECIMATE_CASES = [
    # N, H, W, C, groups
    (2, 6, 10, 8, 2),
    (1, 2, 2, 132, 4),          # one output pixel, 33 channel quads; 33 channels per group: a quad spans groups
]


def _pitched_out(dev, N, Ho, Wo, C):
    return torch.full((N, Ho, Wo, C + 4), SENT).to(dev)


def decimate(dev, N, H, W, C, groups):
    """Modes 3 / 4 keep x[:, 0::2, 0::2] / x[:, 1::2, 1::2]: bit-equal without normalisation; with GroupNorm + SiLU bit-equal to the
    same wrapper's mode-0 result sliced the same way (one gn_xform, one set of coefficients).  Destination pitch C + 4: the pad stays."""
    g = torch.Generator().manual_seed(H * 100 + C)
    x = torch.randn(N, H, W, C, generator=g) * 2.0 + 0.7
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    stats = ops.groupnorm_stats(xd, groups)
    full = ops.groupnorm_apply(xd, stats, gd, bd, silu=True, resample=0, groups=groups).cpu()
    ref_gn = F.silu(F.group_norm(x.permute(0, 3, 1, 2).double(), groups, gamma.double(), beta.double(), 1e-5)).permute(0, 2, 3, 1)
    assert rel_err(full, ref_gn) < TOL                     # (the mode-0 result the decimated ones are compared with is itself right)
    for mode, o in ((3, 0), (4, 1)):
        y = ops.groupnorm_apply(xd, None, None, None, resample=mode, out=_pitched_out(dev, N, H // 2, W // 2, C)).cpu()
        assert torch.equal(y[..., :C], x[:, o::2, o::2]), f"mode {mode}: wrong positions"
        assert _untouched(y[..., C:])
        y = ops.groupnorm_apply(xd, stats, gd, bd, silu=True, resample=mode, groups=groups,
                                out=_pitched_out(dev, N, H // 2, W // 2, C)).cpu()
        assert torch.equal(y[..., :C], full[:, o::2, o::2]), f"mode {mode} with GroupNorm + SiLU"
        assert _untouched(y[..., C:])
        y = ops.groupnorm_apply(xd, None, None, None, resample=mode).cpu()          # the wrapper's own destination: [N, H/2, W/2, C]
        assert tuple(y.shape) == (N, H // 2, W // 2, C) and torch.equal(y, x[:, o::2, o::2])


def decimate_rejects_odd_sizes(dev):
    for shape in ((1, 3, 4, 8), (1, 4, 3, 8)):
        x = torch.randn(*shape).to(dev)
        for mode in (3, 4):
            out = _pitched_out(dev, shape[0], shape[1] // 2, shape[2] // 2, shape[3])
            with pytest.raises(ops._lib.BBDMHipError):
                ops.groupnorm_apply(x, None, None, None, resample=mode, out=out)
            assert _untouched(out.cpu())


def strided_conv_through_decimation(dev):
    """As the plans use the modes: the stride-1 'same' 3x3 convolution followed by mode 4 is the VQGAN Downsample (stride 2 on a
    (0, 1, 0, 1)-padded input), followed by mode 3 the UNet's Downsample(use_conv=True) (stride 2, padding 1)."""
    g = torch.Generator().manual_seed(31)
    N, H, W, Cin, Cout = 2, 8, 12, 32, 64
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05
    b = torch.randn(Cout, generator=g) * 0.1
    full = ops.conv2d_nhwc(x.permute(0, 2, 3, 1).contiguous().to(dev), ops.pack_conv_weight(w.to(dev)), b.to(dev), Cout, 3)
    x64, w64, b64 = x.double(), w.double(), b.double()
    for mode, ref in ((4, F.conv2d(F.pad(x64, (0, 1, 0, 1)), w64, b64, stride=2)), (3, F.conv2d(x64, w64, b64, stride=2, padding=1))):
        y = ops.groupnorm_apply(full, None, None, None, resample=mode).cpu()
        e = rel_err(y.permute(0, 3, 1, 2), ref)
        print(f"3x3 conv + resample {mode} against the stride-2 convolution: rel err {e:.2e}")
        assert e < TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# d. nearest codebook entry
# ---------------------------------------------------------------------------------------------------------------------------------
VQ_CASES = [
    # e_dim, n_e, pixels, ldz, ldq
    (1, 5, 300, 4, 4),
    (2, 1025, 257, 2, 4),           # one code in the second LDS chunk
    (5, 1500, 700, 8, 5),
    (7, 2049, 513, 8, 8),           # three chunks
    (3, 100, 1000, 4, 4),           # the product's call: e_dim 3 at pitch 4
    (6, 300, 256, 6, 6),
]
VQ_GRID_STRIDE_CASE = (1, 3, 4096 * 256 + 300, 1, 1)      # the grid is capped at 4096 workgroups: the second pass of the pixel loop


def _vq_inputs(e_dim, n_e, pixels, ldz, seed=10):
    # (the stream: with 5 codes on a line two random pairs in five are neighbours and their midpoint is a true near-tie -- 7 % of the
    # first case on average, 3 % with this one; _vq_check_indices wants at most 5 % of a case undecided, a property of the inputs)
    g = torch.Generator().manual_seed(e_dim * 10007 + n_e + seed)
    cb = torch.randn(n_e, e_dim, generator=g) * 0.5
    if n_e > 4:
        cb[4] = cb[1]                               # an exact duplicate inside one LDS chunk
    if n_e > 1100:
        cb[1030] = cb[3]                            # ... and in a later chunk
    pick = torch.randint(0, n_e, (pixels,), generator=g)
    if n_e > 4:
        pick[50:58] = 4                             # latents at the duplicates: the first of the equal rows must be returned
    if n_e > 1100:
        pick[58:66] = 1030
    z = cb[pick] + 1e-3 * torch.randn(pixels, e_dim, generator=g)
    ia, ib = torch.randint(0, n_e, (50,), generator=g), torch.randint(0, n_e, (50,), generator=g)
    z[:50] = 0.5 * (cb[ia] + cb[ib])                # midpoints of code pairs: near-ties wherever the two are the nearest codes
    zp = torch.full((pixels, ldz), NAN)
    zp[:, :e_dim] = z
    return cb, z, zp


def _vq_reference(cb, z, chunk=65536):
    """Per pixel, in fp64: the squared distances' minimum, the lowest index attaining it, and the smallest distance to a code whose
    row differs from that one's (bit-identical rows are one code: the kernel evaluates them identically, so the first wins)."""
    n_e = cb.shape[0]
    canon, seen = torch.empty(n_e, dtype=torch.int64), {}
    for j, row in enumerate(cb.tolist()):
        canon[j] = seen.setdefault(tuple(row), j)
    cb64 = cb.double()
    dmin, first, second = [], [], []
    for p0 in range(0, z.shape[0], chunk):
        d = ((z[p0:p0 + chunk].double()[:, None, :] - cb64[None]) ** 2).sum(-1)
        m = d.min(1).values
        f = torch.where(d == m[:, None], torch.arange(n_e)[None], n_e).min(1).values
        other = d.masked_fill(canon[None] == canon[f][:, None], float("inf"))
        dmin.append(m), first.append(f), second.append(other.min(1).values)
    return torch.cat(dmin), torch.cat(first), torch.cat(second)


def _vq_check_indices(cb, z, idx, e_dim, label):
    """With d64 the exact squared distances and bound_p = (e_dim + 3) u (|z|^2 + |e|^2 + 2 sum |z_k e_k|) of the returned code -- the
    fp32 evaluation of (zz + ee) - 2 dot is within that of d64: e_dim roundings in each of zz, ee and the dot product, one in their sum,
    one in the difference --
      * every pixel: d64[returned] - min d64 <= 2 bound_p (both candidates are off by at most bound_p);
      * every pixel whose nearest DIFFERENT code row lies more than 4 bound_p above the minimum: the lowest index attaining the minimum
        (among bit-equal rows the first wins, across LDS chunks too).  Such pixels must be >= 95 % of the case, or the inputs are at
        fault."""
    assert bool(((idx >= 0) & (idx < cb.shape[0])).all())
    dmin, first, second = _vq_reference(cb, z)
    e64, z64 = cb.double()[idx], z.double()
    d_got = ((z64 - e64) ** 2).sum(1)
    bound = (e_dim + 3) * U * ((z64 ** 2).sum(1) + (e64 ** 2).sum(1) + 2 * (z64 * e64).abs().sum(1))
    ratio = float(((d_got - dmin) / (2 * bound)).max())
    forced = second > dmin + 4 * bound
    frac = float(forced.double().mean())
    wrong = int((idx[forced] != first[forced]).sum())
    print(f"vq_nearest {label}: worst (d[returned] - min d) / (2 bound) = {ratio:.3f}; {100 * frac:.2f} % of the pixels forced, "
          f"{wrong} of them wrong")
    assert ratio <= 1.0
    assert frac >= 0.95, "test inputs: too few pixels with a decided answer"
    assert wrong == 0
    return first


def vq_nearest(dev, e_dim, n_e, pixels, ldz, ldq):
    cb, z, zp = _vq_inputs(e_dim, n_e, pixels, ldz)
    zd, cd = zp.to(dev), cb.to(dev)
    idx, zq = ops.vq_nearest(zd, cd, e_dim=e_dim, ldq=ldq, zq_fill=SENT)
    idx, zq = idx.cpu(), zq.cpu()
    _vq_check_indices(cb, z, idx, e_dim, (e_dim, n_e, pixels, ldz, ldq))
    if n_e > 4:
        assert bool((idx[50:58] == 1).all()), "duplicate rows 1 and 4: the first must win"
    if n_e > 1100:
        assert bool((idx[58:66] == 3).all()), "duplicate rows 3 and 1030 (a later chunk): the first must win"
    assert torch.equal(zq[:, :e_dim], cb[idx])
    assert _untouched(zq[:, e_dim:])
    # the reference expression of quantize.py:280-285 in fp32 PyTorch on the near-tie rows: reported, not asserted (its own pick there
    # depends on its host's matmul rounding)
    d32 = torch.sum(z[:50] ** 2, dim=1, keepdim=True) + torch.sum(cb ** 2, dim=1) - 2 * torch.einsum('bd,dn->bn', z[:50], cb.t())
    print(f"    near-tie rows equal to the fp32 PyTorch expression's argmin: {int((idx[:50] == torch.argmin(d32, dim=1)).sum())} / 50")
    only_idx, none = ops.vq_nearest(zd, cd, e_dim=e_dim, ldq=ldq, want_zq=False)
    assert none is None and torch.equal(only_idx.cpu(), idx)
    none, only_zq = ops.vq_nearest(zd, cd, e_dim=e_dim, ldq=ldq, want_idx=False, zq_fill=SENT)
    assert none is None and torch.equal(only_zq.cpu(), zq)


def vq_nearest_grid_stride(dev):
    e_dim, n_e, pixels, ldz, ldq = VQ_GRID_STRIDE_CASE
    cb, z, zp = _vq_inputs(e_dim, n_e, pixels, ldz)
    idx, _ = ops.vq_nearest(zp.to(dev), cb.to(dev), e_dim=e_dim, ldq=ldq, want_zq=False)
    _vq_check_indices(cb, z, idx.cpu(), e_dim, VQ_GRID_STRIDE_CASE)


def vq_nearest_rejects(dev):
    """e_dim outside 1..8 and a z pitch below e_dim are errors."""
    cb = torch.randn(16, 12)
    for e_dim, ldz in ((0, 4), (9, 12), (3, 2)):
        z = torch.randn(40, ldz).to(dev)
        c = cb[:, :max(e_dim, 1)].contiguous().to(dev)
        with pytest.raises(ops._lib.BBDMHipError):
            ops.vq_nearest(z, c, e_dim=e_dim)
        with pytest.raises(ops._lib.BBDMHipError):
            ops.vq_nearest(z, c, e_dim=e_dim, want_zq=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# e. argument checks: an error before any launch, the destination unchanged
# ---------------------------------------------------------------------------------------------------------------------------------
def argument_checks(dev):
    Err = ops._lib.BBDMHipError
    rows, K, R = 36, 36, 20
    bm = torch.randn(1, R, K).to(dev)
    packed = ops.gemm_pack_b(bm, R, K, False)

    def fresh_out(ldo=R):
        return torch.full((1, rows, ldo), SENT).to(dev)

    # K % 4 (with a legal pitch)
    out = fresh_out()
    with pytest.raises(Err):
        ops.gemm_batched(torch.randn(1, rows, 40).to(dev), packed, rows, 34, R, out=out)
    assert _untouched(out.cpu())
    # lda % 4
    out = fresh_out()
    with pytest.raises(Err):
        ops.gemm_batched(torch.randn(1, rows, K + 1).to(dev), packed, rows, K, R, out=out)
    assert _untouched(out.cpu())
    # base pointer 4 bytes off a 16-byte boundary
    out = fresh_out()
    flat = torch.randn(rows * K + 4).to(dev)
    a_off = flat[1:1 + rows * K].view(1, rows, K)
    assert a_off.data_ptr() % 16 == 4 and a_off.is_contiguous()
    with pytest.raises(Err):
        ops.gemm_batched(a_off, packed, rows, K, R, out=out)
    assert _untouched(out.cpu())
    # ldo < R
    out = fresh_out(R - 1)
    with pytest.raises(Err):
        ops.gemm_batched(torch.randn(1, rows, K).to(dev), packed, rows, K, R, out=out)
    assert _untouched(out.cpu())
    # the same call with legal arguments goes through (the rejections above are not a dead wrapper)
    out = fresh_out()
    ops.gemm_batched(torch.randn(1, rows, K).to(dev), packed, rows, K, R, out=out)
    assert not bool((out.cpu() == SENT).any())

    # softmax_rows: ld < T
    s = torch.full((3, 35), SENT).to(dev)
    with pytest.raises(Err):
        ops.softmax_rows(s, 36, 0.37)
    assert _untouched(s.cpu())

    # gemm_pack_b: ldb too small, in both orientations
    for transposed, shape in ((False, (1, R, K - 1)), (True, (1, K, R - 1))):
        pk = torch.full((ops.gemm_packed_b_floats(R, K),), SENT).to(dev)
        with pytest.raises(Err):
            ops.gemm_pack_b(torch.randn(*shape).to(dev), R, K, transposed, packed=pk)
        assert _untouched(pk.cpu())
