"""Shared bodies of the latent-cache tests (the cached q_sample kernels and the channel statistics of csrc/bridge.hip,
bbdm_amd/latent_cache.py, the index path of LatentBrownianBridgeModel.forward): run on the emulated kernels by
tests/test_latent_cache_emu_cpu.py and on the GPU by tests/test_latent_cache_gpu.py -- TEST INFRASTRUCTURE.

Every criterion but the statistics' accuracy is bitwise: the fused gather + normalise + q_sample kernel against the unfused kernels fed
rows that torch gathered (and normalised) on the same device, the cache against ``encode``, the training step on indices against the
training step on the images the rows were encoded from.  The statistics are compared with a float64 evaluation at one fp32 ulp (the
kernel rounds an exact sum once; the float64 reference itself is good to ~1e-16 relative)."""
import argparse
import functools
import math

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset

from fixtures import load_case
from philox_cases import _offset, _stream

SENTINEL = -77.0


def _ns(c):
    ns = argparse.Namespace()
    for k, v in c.items():
        setattr(ns, k, _ns(v) if isinstance(v, dict) else v)
    return ns


def _ptr(t):
    return None if t is None else t.data_ptr()


def _tables(dev):
    from bbdm_amd import bridge_schedule
    tables, _ = bridge_schedule(1000, "linear", 1.0, True, "linear", 200)
    return (torch.tensor(tables[k], dtype=torch.float32, device=dev) for k in ("m_t", "variance_t"))


def _cached(philox, ori, cond, idx_ori, idx_cond, stats, hw, src, t, m_t, var_t, objective, outs):
    """src: (noise,) or (seed, ordinal).  outs: x_t, target, y_out."""
    from bbdm_amd import _lib
    name = "bbdm_bb_q_sample_cached_philox_f32" if philox else "bbdm_bb_q_sample_cached_f32"
    _lib.call(name, ori.data_ptr(), cond.data_ptr(), ori.shape[0], idx_ori.data_ptr(), idx_cond.data_ptr(),
              *(_ptr(s) for s in (stats or [None] * 4)), hw, *(s.data_ptr() for s in src), t.data_ptr(), m_t.data_ptr(),
              var_t.data_ptr(), *(o.data_ptr() for o in outs), idx_ori.shape[0], ori[0].numel(), objective, _stream(ori.device))


def _unfused(philox, a, b, src, t, m_t, var_t, objective, outs):
    from bbdm_amd import _lib
    name = "bbdm_bb_q_sample_philox_f32" if philox else "bbdm_bb_q_sample_f32"
    _lib.call(name, a.data_ptr(), b.data_ptr(), *(s.data_ptr() for s in src), t.data_ptr(), m_t.data_ptr(), var_t.data_ptr(),
              *(o.data_ptr() for o in outs), a.shape[0], a[0].numel(), objective, _stream(a.device))


M_ROWS = 7
IDX_ORI = [3, 0, 6, 3, 1]              # a repeat, 0 and M - 1, out of order
IDX_COND = [6, 2, 0, 5, 6]             # != idx_ori in every slot


def _kernel_inputs(dev, shape, off):
    g = torch.Generator().manual_seed(31)
    ori, cond = (_offset(torch.randn((M_ROWS,) + shape, generator=g).to(dev), off) for _ in range(2))
    noise = _offset(torch.randn((len(IDX_ORI),) + shape, generator=g).to(dev), off)
    t = torch.tensor([0, 999, 412, 57, 640], dtype=torch.int64, device=dev)
    seed = torch.tensor([1, 2 ** 35 + 2, -4, 3, 99], dtype=torch.int64, device=dev)
    ordinal = torch.tensor([0, 2 ** 32 + 1, 17, 17, 5], dtype=torch.int64, device=dev)
    # means of a few tenths, stds in [0.5, 4]
    stats = [torch.tensor(v, dtype=torch.float32, device=dev) for v in
             ([0.3, -0.2, 0.45], [0.5, 4.0, 1.7], [-0.35, 0.25, 0.1], [2.9, 0.75, 3.3])]
    return ori, cond, noise, t, seed, ordinal, stats


def kernel_equals_unfused(dev, shape, off, philox):
    """1. M = 7 rows, N = 5 indices: the cached kernel equals the unfused kernel fed the rows torch gathered -- and, with statistics,
    ``(z - mean) / std`` evaluated by torch on the same device -- torch.equal on x_t and target, and y_out equals the gathered
    (normalised) condition rows; objectives 0, 1, 2.  ``off`` = 1: every tensor starts 4 bytes past its allocation; (3, 321) has
    per_sample % 4 != 0, hw % 4 != 0 and groups that straddle channels."""
    ori, cond, noise, t, seed, ordinal, stats = _kernel_inputs(dev, shape, off)
    m_t, var_t = _tables(dev)
    io, ic = (torch.tensor(v, dtype=torch.int64, device=dev) for v in (IDX_ORI, IDX_COND))
    C, hw = shape[0], int(np.prod(shape[1:]))
    assert ori[0].numel() == C * hw
    src = (seed, ordinal) if philox else (noise,)
    bc = (1, C) + (1,) * (len(shape) - 1)
    checked = 0
    for st in (None, stats):
        a, b = ori[io], cond[ic]
        if st is not None:
            a = (a - st[0].view(bc)) / st[1].view(bc)
            b = (b - st[2].view(bc)) / st[3].view(bc)
        a, b = _offset(a, off), _offset(b, off)
        for objective in (0, 1, 2):
            ref = [torch.full_like(a, SENTINEL) for _ in range(2)]
            _unfused(philox, a, b, src, t, m_t, var_t, objective, ref)
            got = [_offset(torch.full_like(a, SENTINEL), off) for _ in range(3)]
            _cached(philox, ori, cond, io, ic, st, hw, src, t, m_t, var_t, objective, got)
            for x, want, name in zip(got, ref + [b], ("x_t", "target", "y_out")):
                assert bool(torch.isfinite(want).all())
                assert torch.equal(x, want), (name, objective, st is not None, float((x - want).abs().max()))
                checked += 1
    assert checked == 18


def ragged_group_follows_the_formula(dev, philox):
    """1b. The element route with a ragged last group (N = 3, per_sample = hw = 7, statistics on) against torch fp32 tensor ops in
    the reference's order: (z - mean) / std (LatentBrownianBridgeModel.py:92-97), then q_sample (BrownianBridgeModel.py:128-146).

    Bound.  The kernel evaluates the same IEEE fp32 operations (no contraction; the division and sqrtf are correctly rounded by
    default), so the results differ at most by a last-place difference of the division or the square root: 2^-23 of a term each.
    y_out is one subtraction and one division: <= 2 * 2^-23 relative.  x_t and the target take two such rows and sqrt(var):
    <= 8 * 2^-23 * S elementwise, S the sum of the terms' absolute values."""
    from bbdm_amd import philox_normal
    g = torch.Generator().manual_seed(33)
    M, N, shape = 4, 3, (1, 7)
    ori, cond, noise = torch.randn((M,) + shape, generator=g), torch.randn((M,) + shape, generator=g), torch.randn((N,) + shape, generator=g)
    io, ic, t = [2, 0, 3], [1, 3, 0], [0, 999, 412]
    stats = [torch.tensor([v], dtype=torch.float32) for v in (0.3, 1.7, -0.35, 0.75)]
    m_t, var_t = _tables(dev)
    seed = torch.tensor([1, 2 ** 35 + 2, -4], dtype=torch.int64, device=dev)
    ordinal = torch.tensor([0, 2 ** 32 + 1, 17], dtype=torch.int64, device=dev)
    if philox:
        noise = philox_normal(shape, seed, ordinal, domain=1).cpu()
    src = (seed, ordinal) if philox else (noise.to(dev),)
    m = m_t.cpu()[t].view(N, 1, 1)
    sig = torch.sqrt(var_t.cpu()[t]).view(N, 1, 1)
    a, b = (ori[io] - stats[0]) / stats[1], (cond[ic] - stats[2]) / stats[3]
    eps = 2.0 ** -23
    for objective in (0, 1, 2):
        got = [torch.full((N,) + shape, SENTINEL, device=dev) for _ in range(3)]
        _cached(philox, ori.to(dev), cond.to(dev), *(torch.tensor(v, dtype=torch.int64, device=dev) for v in (io, ic)),
                [s.to(dev) for s in stats], 7, src, torch.tensor(t, dtype=torch.int64, device=dev), m_t, var_t, objective, got)
        x_t, target, y_out = (o.cpu() for o in got)
        ref_x, s_x = (1.0 - m) * a + m * b + sig * noise, (1.0 - m) * a.abs() + m * b.abs() + sig * noise.abs()
        if objective == 0:
            ref_t, s_t = m * (b - a) + sig * noise, m * (b.abs() + a.abs()) + sig * noise.abs()
        elif objective == 1:
            ref_t, s_t = noise, noise.abs()
        else:
            ref_t, s_t = b - a, b.abs() + a.abs()
        ey = float(((y_out - b).abs() / b.abs()).max())
        ex, et = float(((x_t - ref_x).abs() / s_x).max()), float(((target - ref_t).abs() / s_t).max())
        print(f"objective {objective} philox {philox}: y_out {ey / eps:.2f}, x_t {ex / eps:.2f}, target {et / eps:.2f} x 2^-23 (bars 2, 8, 8)")
        assert ey <= 2 * eps and ex <= 8 * eps and et <= 8 * eps, (objective, ey, ex, et)


def out_of_range_rows_are_nan(dev, shape, off, philox):
    """2. Indices -1 and M: NaN rows in all three outputs for those images, every other image bit-equal to the in-range run."""
    ori, cond, noise, t, seed, ordinal, stats = _kernel_inputs(dev, shape, off)
    m_t, var_t = _tables(dev)
    C, hw = shape[0], int(np.prod(shape[1:]))
    src = (seed, ordinal) if philox else (noise,)
    io, ic = (torch.tensor(v, dtype=torch.int64, device=dev) for v in (IDX_ORI, IDX_COND))
    bad_o, bad_c = io.clone(), ic.clone()
    bad_o[1] = -1                       # image 1: its ori index; image 2: its cond index
    bad_c[2] = M_ROWS
    for st in (None, stats):
        good = [_offset(torch.full((5,) + shape, SENTINEL, device=dev), off) for _ in range(3)]
        _cached(philox, ori, cond, io, ic, st, hw, src, t, m_t, var_t, 0, good)
        got = [_offset(torch.full((5,) + shape, SENTINEL, device=dev), off) for _ in range(3)]
        _cached(philox, ori, cond, bad_o, bad_c, st, hw, src, t, m_t, var_t, 0, got)
        for x, want in zip(got, good):
            assert bool(torch.isnan(x[1]).all()) and bool(torch.isnan(x[2]).all())
            assert torch.equal(x[[0, 3, 4]], want[[0, 3, 4]]) and bool(torch.isfinite(want).all())


# --------------------------------------------------------------------------------------------------------------
def _ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _stats_rows():
    g = torch.Generator().manual_seed(41)
    std = torch.tensor([0.5, 1.0, 2.0, 0.7, 1.3, 0.9, 1.6, 0.6])
    off = torch.tensor([0.0, 1.0, -5.0, 50.0, -50.0, 20.0, 0.3, -12.0]) * std      # up to 50 x the std: the cancellation case
    return torch.randn(37, 8, 8, 8, generator=g) * std.view(1, 8, 1, 1) + off.view(1, 8, 1, 1)


def channel_stats(dev, nan_row=False):
    """3. M = 37 rows of (8, 8, 8): the mean within 1 fp32 ulp of the float64 mean, the std within 1 ulp of the float64 value computed
    about the same fp32-rounded mean (the var likewise); bit-identical after permuting the rows and for every split of the rows over
    blocks.  ``nan_row``: one NaN makes that channel's three outputs NaN and leaves the others' bits."""
    from bbdm_amd.latent_cache import channel_stats as stats
    z = _stats_rows().to(dev)
    mean, var, std = stats(z)
    z64 = z.double().cpu()
    ref_mean = z64.mean(dim=(0, 2, 3))
    ref_var = ((z64 - mean.double().cpu().view(1, 8, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    for c in range(8):
        em = abs(float(mean[c].double().cpu()) - float(ref_mean[c]))
        ev = abs(float(var[c].double().cpu()) - float(ref_var[c]))
        es = abs(float(std[c].double().cpu()) - math.sqrt(float(ref_var[c])))
        print(f"channel {c}: mean {float(mean[c]):+.6e} err {em / _ulp32(ref_mean[c]):.3f} ulp, var err {ev / _ulp32(ref_var[c]):.3f} ulp, "
              f"std {float(std[c]):.6e} err {es / _ulp32(math.sqrt(float(ref_var[c]))):.3f} ulp")
        assert em <= _ulp32(ref_mean[c]) and ev <= _ulp32(ref_var[c]) and es <= _ulp32(math.sqrt(float(ref_var[c])))
    perm = torch.randperm(37, generator=torch.Generator().manual_seed(42))
    assert not torch.equal(perm, torch.arange(37))
    for other in [stats(z[perm.to(dev)].contiguous())] + [stats(z, row_blocks=rb) for rb in (1, 5, 36, 37, 4096)]:
        for a, b in zip(other, (mean, var, std)):
            assert torch.equal(a, b)
    if nan_row:
        z2 = z.clone()
        z2[5, 3, 2, 2] = float("nan")
        got = stats(z2)
        keep = [c for c in range(8) if c != 3]
        for a, b in zip(got, (mean, var, std)):
            assert bool(torch.isnan(a[3])) and torch.equal(a[keep], b[keep])


# --------------------------------------------------------------------------------------------------------------
class Pairs(Dataset):
    """A dozen seeded in-memory pairs, items ((x, name), (x_cond, name)) like the reference's paired datasets."""

    def __init__(self, n=12, noisy=False):
        g = torch.Generator().manual_seed(51)
        self.x = torch.randn(n, 3, 32, 32, generator=g).clamp(-1, 1)
        self.c = torch.randn(n, 3, 32, 32, generator=g).clamp(-1, 1)
        self.noisy = noisy

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        x = self.x[i] + 1e-3 * torch.randn(3, 32, 32) if self.noisy else self.x[i]
        return (x, f"{i:03d}"), (self.c[i], f"{i:03d}_cond")


def latent_model(dev):
    """The tiny latent configuration of tests/test_latent_gpu.py::test_latent_with_builtin_first_stage (32^2 images, latent 8x8x8,
    nocond)."""
    import bbdm_amd
    rec = load_case("tiny_nocond")
    dd = dict(double_z=False, z_channels=8, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2, 2),
              num_res_blocks=1, attn_resolutions=[], dropout=0.0)
    cfg = _ns({"BB": {"params": dict(rec["bb_params"], UNetParams=rec["unet_params"])},
               "VQGAN": {"params": {"ckpt_path": None, "embed_dim": 8, "n_embed": 128, "ddconfig": dd,
                                    "lossconfig": {"target": "torch.nn.Identity"}}},
               "normalize_latent": False, "latent_before_quant_conv": False})
    assert rec["unet_params"]["condition_key"] == "nocond"
    torch.manual_seed(4)
    m = bbdm_amd.LatentBrownianBridgeModel(cfg).to(dev)
    m.denoise_fn.load_state_dict({k[len("denoise_fn."):]: v for k, v in rec["state_dict"].items() if k.startswith("denoise_fn.")})
    return m.train()


@functools.lru_cache(maxsize=None)
def shared(dev):
    """(model, dataset, cache built with batch_size 4) -- built once per device and left unchanged by the tests (each one restores the
    attributes it sets)."""
    from bbdm_amd import LatentCache
    m, ds = latent_model(dev), Pairs()
    return m, ds, LatentCache.build(m, ds, batch_size=4)


def cache_equals_encode(dev, tmp_path):
    """4. Rows == encode(normalize=False) of the same consecutive batches; save / load round-trips bitwise; load against a perturbed
    quant_conv raises; verify catches a dataset with fresh noise per fetch; build refuses a model with a conditioning stage."""
    from bbdm_amd import LatentCache
    m, ds, cache = shared(dev)
    assert tuple(cache.ori.shape) == (12, 8, 8, 8) and cache.ori.device.type == dev.type and len(cache) == 12
    assert cache.names == [(f"{i:03d}", f"{i:03d}_cond") for i in range(12)]
    for r in range(0, 12, 4):
        assert torch.equal(cache.ori[r:r + 4], m.encode(ds.x[r:r + 4].to(dev), cond=False, normalize=False))
        assert torch.equal(cache.cond[r:r + 4], m.encode(ds.c[r:r + 4].to(dev), cond=True, normalize=False))
    assert not torch.equal(cache.ori, cache.cond)
    path = tmp_path / "latents.pt"
    cache.save(path)
    back = LatentCache.load(path, m)
    assert torch.equal(back.ori, cache.ori) and torch.equal(back.cond, cache.cond) and back.ori.device == cache.ori.device
    assert back.names == cache.names and back.fingerprint == cache.fingerprint
    w = m.vqgan.quant_conv.weight
    keep = w.detach().clone()
    try:
        with torch.no_grad():
            w[0, 0, 0, 0] += 1e-3
        with pytest.raises(ValueError, match="fingerprint"):
            LatentCache.load(path, m)
    finally:
        with torch.no_grad():
            w.copy_(keep)
    LatentCache.load(path, m)
    with pytest.raises(ValueError, match="differs between two fetches"):
        LatentCache.build(m, Pairs(noisy=True), batch_size=4)
    m.cond_stage_model = torch.nn.Identity()
    try:
        with pytest.raises(ValueError, match="latent cache cannot serve"):
            LatentCache.build(m, ds, batch_size=4)
        with pytest.raises(ValueError, match="latent cache cannot serve"):
            m.attach_latent_cache(cache)
    finally:
        m.cond_stage_model = None
    mean_std = cache.mean_std()
    assert all(tuple(v.shape) == (1, 8, 1, 1) and v.dtype == torch.float32 and v.device == cache.ori.device for v in mean_std)
    assert torch.allclose(mean_std[0].cpu(), cache.ori.cpu().mean(dim=(0, 2, 3), keepdim=True), atol=1e-5)
    assert torch.allclose(mean_std[3].cpu(), cache.cond.cpu().std(dim=(0, 2, 3), keepdim=True, unbiased=False), rtol=1e-4)


def _raise(*a, **k):
    raise AssertionError("encoder work on the index path")


def _step(m, fn):
    for p in m.denoise_fn.parameters():
        p.grad = None
    loss, log = fn()
    loss.backward()
    grads = {k: p.grad.clone() for k, p in m.denoise_fn.named_parameters()}
    assert len(grads) > 0 and all(g is not None for g in grads.values())
    return loss.detach().clone(), log["x0_recon"].clone(), grads


def training_step_index_equals_image(dev, monkeypatch, normalize, loss_type, seeded):
    """5. From the same generator state, the micro-step on the images of batch rows 4..7 and on their indices: equal loss, equal
    x0_recon, torch.equal gradients on every UNet parameter; the encoder is patched to raise during the index call."""
    m, ds, cache = shared(dev)
    x, c = ds.x[4:8].to(dev), ds.c[4:8].to(dev)
    idx = torch.arange(4, 8, dtype=torch.int64, device=dev)
    monkeypatch.setattr(m, "loss_type", loss_type)
    monkeypatch.setattr(m.model_config, "normalize_latent", normalize)
    if normalize:
        cache.install_stats(m)
        assert tuple(m.ori_latent_std.shape) == (1, 8, 1, 1)
    seeds, ordinal = [900 + 3 * k for k in range(4)], 6
    t = torch.tensor([7, 999, 0, 431], dtype=torch.int64, device=dev)

    def image_path():
        torch.manual_seed(77)
        if not seeded:
            return m(x, c)
        with torch.no_grad():
            a, b = m.encode(x, cond=False), m.encode(c, cond=True)
        return m.p_losses(a, b, None, t, seeds=seeds, ordinals=ordinal)

    def index_path():
        torch.manual_seed(77)
        return m(idx, idx) if not seeded else m.p_losses_cached(idx, idx, t, seeds=seeds, ordinals=ordinal)

    try:
        m.attach_latent_cache(cache)
        want = _step(m, image_path)
        print(f"loss image path {float(want[0]):.9g}")
        with monkeypatch.context() as mp:
            if hasattr(m.vqgan, "encode_latent"):
                mp.setattr(m.vqgan, "encode_latent", _raise)
            mp.setattr(m.vqgan.encoder, "forward", _raise)
            with pytest.raises(AssertionError, match="encoder work"):
                m.encode(x, cond=False)
            got = _step(m, index_path)
        print(f"loss index path {float(got[0]):.9g}")
        assert bool(torch.isfinite(want[0])) and torch.equal(got[0], want[0]), (float(got[0]), float(want[0]))
        assert torch.equal(got[1], want[1])
        for k, g in want[2].items():
            assert torch.equal(got[2][k], g), k
        assert any(float(g.abs().max()) > 0 for g in want[2].values())
    finally:
        m.detach_latent_cache()
        for p in m.denoise_fn.parameters():
            p.grad = None
        for name in ("ori_latent_mean", "ori_latent_std", "cond_latent_mean", "cond_latent_std"):
            if hasattr(m, name):
                delattr(m, name)


def float_inputs_keep_their_path(dev):
    """5. (last bullet) A float-input call after attach_latent_cache equals the call before it: loss and x0_recon, bitwise."""
    m, ds, cache = shared(dev)
    x, c = ds.x[4:8].to(dev), ds.c[4:8].to(dev)
    runs = []
    try:
        for attach in (False, True):
            if attach:
                m.attach_latent_cache(cache)
            torch.manual_seed(78)
            with torch.no_grad():
                loss, log = m(x, c)
            runs.append((loss.clone(), log["x0_recon"].clone()))
    finally:
        m.detach_latent_cache()
    assert bool(torch.isfinite(runs[0][0])) and torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def index_input_errors(dev):
    """2. (model) CPU indices out of range raise IndexError before any launch; an integer tensor that is not [N] raises ValueError;
    integer input without an attached cache raises RuntimeError."""
    m, ds, cache = shared(dev)
    m.detach_latent_cache()
    with pytest.raises(RuntimeError, match="attach_latent_cache"):
        m(torch.arange(4), torch.arange(4))
    m.attach_latent_cache(cache)
    try:
        for bad in ([0, 12, 1, 2], [0, -1, 1, 2]):
            with pytest.raises(IndexError):
                m(torch.tensor(bad), torch.arange(4))
            with pytest.raises(IndexError):
                m(torch.arange(4), torch.tensor(bad))
        with pytest.raises(ValueError):
            m(torch.zeros(4, 1, dtype=torch.int64), torch.zeros(4, 1, dtype=torch.int64))
        with pytest.raises(ValueError):
            m(torch.arange(4), torch.arange(3))
    finally:
        m.detach_latent_cache()


def runner_seam(dev):
    """6. A DataLoader over CachedPairs feeds the runner's loss_fn (BBDMRunner.py:164-176, restated below as far as the model is
    concerned, the way tests/test_runner_integration.py restates the runner): finite loss, equal to the model-level call on the same
    indices."""
    from bbdm_amd import CachedPairs
    m, ds, cache = shared(dev)
    config = argparse.Namespace(training=argparse.Namespace(device=[dev]))

    def loss_fn(net, batch):
        (x, x_name), (x_cond, x_cond_name) = batch
        x = x.to(config.training.device[0])
        x_cond = x_cond.to(config.training.device[0])
        loss, additional_info = net(x, x_cond)
        return loss, x_name, x_cond_name

    pairs = CachedPairs(ds, names=cache.names)
    assert len(pairs) == 12
    (i5, n5), (j5, c5) = CachedPairs(ds)[5]                 # without names: read from the dataset, the same item
    (a5, an5), (b5, bn5) = pairs[5]
    assert int(i5) == int(j5) == int(a5) == int(b5) == 5 and (n5, c5) == (an5, bn5) == ("005", "005_cond") and a5.dtype == torch.int64
    batches = list(DataLoader(pairs, batch_size=4, shuffle=False))
    assert len(batches) == 3
    batch = batches[1]
    assert batch[0][0].dtype == torch.int64 and batch[0][0].tolist() == [4, 5, 6, 7] and list(batch[1][1]) == [f"{i:03d}_cond" for i in range(4, 8)]
    m.attach_latent_cache(cache)
    try:
        torch.manual_seed(5)
        loss, names, cond_names = loss_fn(m, batch)
        assert list(names) == [f"{i:03d}" for i in range(4, 8)]
        loss.backward()                                     # (before the next forward: the training plan keeps one set of activations)
        assert all(p.grad is not None for p in m.get_parameters())
        torch.manual_seed(5)
        direct, _ = m(torch.arange(4, 8, device=dev), torch.arange(4, 8, device=dev))
        assert bool(torch.isfinite(loss)) and torch.equal(loss.detach(), direct.detach())
    finally:
        m.detach_latent_cache()
        for p in m.denoise_fn.parameters():
            p.grad = None
