"""Shared bodies of the evaluation-metric tests (bbdm_amd/metrics.py, csrc/metrics.hip): run on the CPU-emulated kernels by
tests/test_metrics_emu_cpu.py and on the GPU by tests/test_metrics_gpu.py -- TEST INFRASTRUCTURE.

Every reference is written out here in torch / numpy on the CPU:
* pair sums -- numpy int64 sums (the kernel's integers must be equal);
* SSIM      -- float64 ``F.conv2d`` with the 2-D window w (x) w (the kernel applies two 11-tap passes), bar 1e-10 absolute per image:
  the worst case is the cancellation in sigma^2 = E[x^2] - mu^2, about 22 roundings x 65025 x 2^-53 = 1.6e-10 against the smallest
  denominator C2 = 58.5, i.e. about 3e-12 per factor, four factors, and a margin (an fp32-moment implementation gives 2-3e-8);
* diversity -- the fp32 formula of evaluation/diversity.py:26-35 restated in torch (division and square root correctly rounded: see
  ``diversity_reference`` for the root), the standard deviations summed with ``math.fsum`` and divided in float64; bar 4 ulp of
  float64 (the limb fold rounds twice, the division a third time).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

SHAPES = [(3, 11, 11, 3), (2, 13, 19, 1), (3, 37, 45, 3), (1, 256, 256, 3)]          # (N, H, W, C); the SSIM tile is 16 x 32 positions
SSIM_BAR = 1e-10


def _rand_u8(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def pair_inputs(shape, kind="random"):
    """(a, b) uint8 [N, H, W, C] on the CPU (computed once per case and shared; never modified)."""
    a = _rand_u8(shape, 17 + sum(shape))
    if kind == "random":
        b = _rand_u8(shape, 91 + sum(shape))
    elif kind == "flat":                     # bright flat images: the cancellation-heavy case
        a, b = torch.full(shape, 254, dtype=torch.uint8), torch.full(shape, 255, dtype=torch.uint8)
    elif kind == "pm2":                      # differ by +-2 everywhere
        a = a.clamp(2, 253)
        sign = _rand_u8(shape, 5).to(torch.int16) % 2 * 4 - 2
        b = (a.to(torch.int16) + sign).to(torch.uint8)
    elif kind == "same":
        b = a.clone()
    else:
        raise KeyError(kind)
    return a, b


def offset_view(t, offset, dev):
    """The same values on ``dev`` in a buffer whose data pointer is ``offset`` bytes past an allocation boundary."""
    buf = torch.empty(t.numel() + offset + 16, dtype=torch.uint8, device=dev)
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + offset
    return v


# ---- case 1 ------------------------------------------------------------------------------------------------------------------
def pair_sums_exact(dev, shape):
    from bbdm_amd import metrics
    a, b = pair_inputs(shape)
    d = a.numpy().astype(np.int64) - b.numpy().astype(np.int64)
    ref = np.stack([np.abs(d).reshape(shape[0], -1).sum(1), (d * d).reshape(shape[0], -1).sum(1)], 1)
    count = float(shape[1] * shape[2] * shape[3])
    views = [(a.to(dev), b.to(dev)), (offset_view(a, 4, dev), b.to(dev)), (offset_view(a, 4, dev), offset_view(b, 4, dev)),
             (a.to(dev), offset_view(b, 1, dev))]                  # 16-byte words; 4-byte words; 16-byte words behind a head; bytes
    for va, vb in views:
        sums = metrics._pair_sums_raw(va, vb)
        assert sums.dtype == torch.int64 and np.array_equal(sums.cpu().numpy(), ref), (shape, va.data_ptr() % 16, vb.data_ptr() % 16)
    got = metrics.pair_metrics(*views[1])
    for n in range(shape[0]):
        mae, mse = np.float64(ref[n, 0]) / count, np.float64(ref[n, 1]) / count
        assert got["mae"].dtype == torch.float64
        assert float(got["mae"][n]) == float(mae) and float(got["mse"][n]) == float(mse)
        assert float(got["psnr"][n]) == 10.0 * math.log10(65025.0 / float(mse))
    same = metrics.pair_metrics(a.to(dev), a.clone().to(dev))
    assert all(v == 0.0 for v in same["mae"].tolist()) and all(v == 0.0 for v in same["mse"].tolist())
    assert all(v == math.inf for v in same["psnr"].tolist())


# ---- case 2 ------------------------------------------------------------------------------------------------------------------
def ssim_reference(a, b):
    """float64 conv2d with the 2-D window; a, b uint8 [N, H, W, C] -> float64 [N]."""
    from bbdm_amd import metrics
    w = torch.tensor(metrics.ssim_window(), dtype=torch.float64)
    C = a.shape[3]
    k = torch.outer(w, w).expand(C, 1, 11, 11).contiguous()
    x, y = a.permute(0, 3, 1, 2).double(), b.permute(0, 3, 1, 2).double()
    win = lambda t: F.conv2d(t, k, groups=C)
    mx, my = win(x), win(y)
    sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    m = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return m.flatten(1).mean(1)


@functools.lru_cache(maxsize=None)
def ssim_expected(shape, kind):
    return ssim_reference(*pair_inputs(shape, kind))


def ssim_matches(dev, shape, kind):
    from bbdm_amd import metrics
    a, b = pair_inputs(shape, kind)
    got = metrics.pair_metrics(a.to(dev), b.to(dev))["ssim"]
    ref = torch.ones(shape[0], dtype=torch.float64) if kind == "same" else ssim_expected(shape, kind)
    err = (got - ref).abs()
    print(f"ssim {shape} {kind}: max abs err {float(err.max()):.3e} (bar {SSIM_BAR:g}); values {got.tolist()}")
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[0],)
    assert bool((err <= SSIM_BAR).all()), (shape, kind, err.tolist())


def ssim_rejects_small(dev):
    from bbdm_amd import _lib, metrics
    import pytest
    for shape in ((1, 10, 16, 3), (1, 16, 10, 3)):
        a = _rand_u8(shape, 1).to(dev)
        with pytest.raises(_lib.BBDMHipError):
            metrics.pair_metrics(a, a)


# ---- case 3 ------------------------------------------------------------------------------------------------------------------
DIVERSITY_SHAPES = [(1, 1, 11, 11, 3), (2, 2, 16, 16, 3), (3, 5, 13, 19, 3), (2, 5, 32, 32, 3), (1, 5, 37, 45, 3)]   # (M, S, H, W, C)


def diversity_reference(x):
    """x uint8 [M, S, H, W, C] -> list of M Python floats: evaluation/diversity.py:26-35 in fp32, then fsum / count in float64."""
    out = []
    for m in range(x.shape[0]):
        imgs = [x[m, j].to(torch.float32) for j in range(x.shape[1])]
        S = len(imgs)
        mean = torch.zeros_like(imgs[0])
        for j in range(S):
            mean = mean + imgs[j]
        mean = mean / S
        var = torch.zeros_like(imgs[0])
        for j in range(S):
            var = var + (imgs[j] - mean) ** 2
        var = var / S
        # the CORRECTLY ROUNDED fp32 square root the kernel is specified with: the float64 root of an fp32 value, rounded to fp32 (53 >=
        # 2 * 24 + 2 bits: the double rounding cannot show).  torch.sqrt on an fp32 CPU tensor is a vectorised routine that is 1 ulp
        # low for about 0.65 % of arguments on the torch build these tests were written with -- the reference's own error, which
        # would cost ~3e-10 relative in the sum, far above the 4 ulp asked here.
        std = torch.sqrt(var.double()).to(torch.float32)
        assert std.dtype == torch.float32 and var.dtype == torch.float32 and mean.dtype == torch.float32
        out.append(math.fsum(std.flatten().double().tolist()) / float(std.numel()))
    return out


def diversity_matches(dev, shape):
    from bbdm_amd import metrics
    x = _rand_u8(shape, 29 + sum(shape))
    ref = diversity_reference(x)
    views = [x.to(dev)]
    if shape == DIVERSITY_SHAPES[1]:
        views.append(offset_view(x, 1, dev))                       # H W C % 4 == 0 behind an odd pointer: the byte kernel
    for v in views:
        per, mean = metrics.diversity(v)
        assert per.dtype == torch.float64 and tuple(per.shape) == (shape[0],)
        for m in range(shape[0]):
            ulps = abs(float(per[m]) - ref[m]) / math.ulp(ref[m]) if ref[m] else abs(float(per[m]))
            print(f"diversity {shape} m={m}: {float(per[m])!r} vs {ref[m]!r}: {ulps:g} ulp")
            assert ulps <= 4, (shape, m, float(per[m]), ref[m])
        assert mean == float(per.mean())
    if shape[1] == 1:
        assert all(v == 0.0 for v in per.tolist())


def diversity_of_identical_samples_is_zero(dev):
    from bbdm_amd import metrics
    for S in (2, 3, 5, 7):
        one = _rand_u8((2, 1, 13, 19, 3), 40 + S)
        one.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)         # every byte value
        per, mean = metrics.diversity(one.expand(2, S, 13, 19, 3).contiguous().to(dev))
        assert per.tolist() == [0.0, 0.0] and mean == 0.0, (S, per.tolist())


def float_input_is_quantised_like_the_png_writer(dev):
    """fp32 [N, C, H, W] input goes through the egress quantisation: same numbers as the uint8 images it produces."""
    from bbdm_amd import egress, metrics
    g = torch.Generator().manual_seed(8)
    x, y = (torch.randn(2, 3, 13, 19, generator=g).mul(0.6).to(dev) for _ in range(2))
    a = metrics.pair_metrics(x, y)
    b = metrics.pair_metrics(egress._to_u8_device(x, True), egress._to_u8_device(y, True))
    assert all(torch.equal(a[k], b[k]) for k in ("mae", "mse", "psnr", "ssim"))
    s = torch.randn(2, 3, 3, 13, 19, generator=g).mul(0.6).to(dev)
    u = egress._to_u8_device(s.flatten(0, 1), True).view(2, 3, 13, 19, 3)
    assert torch.equal(metrics.diversity(s)[0], metrics.diversity(u)[0])
    assert not torch.equal(metrics.pair_metrics(x, y, to_normal=False)["mse"], a["mse"])


# ---- case 4 ------------------------------------------------------------------------------------------------------------------
def raw_cells_repeat(dev, one_at_a_time):
    from bbdm_amd import metrics
    shape = SHAPES[2]
    a, b = (t.to(dev) for t in pair_inputs(shape))
    s1, c1 = metrics._pair_sums_raw(a, b), metrics._ssim_raw(a, b)
    s2, c2 = metrics._pair_sums_raw(a, b), metrics._ssim_raw(a, b)
    assert torch.equal(s1, s2) and torch.equal(c1, c2)
    x = _rand_u8((3, 5, 37, 45, 3), 77).to(dev)
    d1, d2 = metrics._diversity_raw(x), metrics._diversity_raw(x)
    assert torch.equal(d1, d2)
    if one_at_a_time:                           # the same images alone: another grid, the same cells
        for n in range(shape[0]):
            an, bn = a[n:n + 1].clone(), b[n:n + 1].clone()
            assert torch.equal(metrics._pair_sums_raw(an, bn)[0], s1[n]) and torch.equal(metrics._ssim_raw(an, bn)[0], c1[n]), n
        for m in range(x.shape[0]):
            assert torch.equal(metrics._diversity_raw(x[m:m + 1].clone())[0], d1[m]), m
        whole, parts = metrics.pair_metrics(a, b), [metrics.pair_metrics(a[n:n + 1], b[n:n + 1]) for n in range(shape[0])]
        assert torch.equal(whole["ssim"], torch.cat([p["ssim"] for p in parts]))
        assert torch.equal(metrics.diversity(x)[0], torch.cat([metrics.diversity(x[m:m + 1])[0] for m in range(x.shape[0])]))


# ---- cases 5 and 6 -----------------------------------------------------------------------------------------------------------
def _same_result(r1, r2):
    for k in ("diversity", "psnr", "ssim", "mae"):
        assert r1[k] == r2[k], (k, r1[k], r2[k])
    for k in ("diversity_per_condition", "psnr_per_sample", "ssim_per_sample", "mae_per_sample", "mse_per_sample"):
        assert torch.equal(r1[k], r2[k]), k


def files_equal_tensors(dev, tmp_path):
    """3 conditions x 2 samples at 16 x 16 written by ImageWriter in sample_to_eval's layout: the metrics of the files are exactly the
    metrics of the fp32 tensors."""
    from bbdm_amd import egress, metrics
    g = torch.Generator().manual_seed(12)
    M, S = 3, 2
    samples = torch.randn(M, S, 3, 16, 16, generator=g).mul(0.6).to(dev)
    gts = torch.randn(M, 3, 16, 16, generator=g).mul(0.6).to(dev)
    res, gt = tmp_path / "200", tmp_path / "ground_truth"
    gt.mkdir()
    ev = metrics.SetEvaluator(S)
    with egress.ImageWriter(workers=2) as w:
        for m in range(M):
            (res / str(m)).mkdir(parents=True)
            w.submit(samples[m], str(res / str(m)), [f"output_{j}.png" for j in range(S)])
            ev.add_target(m, gts[m])
            for j in range(S):
                ev.add_sample(m, j, samples[m, j])
        w.submit(gts, str(gt), [f"{m}.png" for m in range(M)])
    from_tensors = ev.result()
    from_files = metrics.metrics_from_dirs(str(res), str(gt), S, device=dev)
    _same_result(from_tensors, from_files)
    assert from_files["conditions"] == ["0", "1", "2"] and -1.0 < from_files["ssim"] < 1.0 and from_files["diversity"] > 0.0


def _check_against_assembled(ev_result, samples_u8, targets_u8, S):
    """``samples_u8`` [M, S, H, W, C], ``targets_u8`` [Mt, H, W, C] for the first Mt conditions."""
    from bbdm_amd import metrics
    per, mean = metrics.diversity(samples_u8)
    assert torch.equal(ev_result["diversity_per_condition"], per) and ev_result["diversity"] == mean
    Mt = targets_u8.shape[0]
    pm = metrics.pair_metrics(samples_u8[:Mt].flatten(0, 1), targets_u8.repeat_interleave(S, 0))
    for k in ("psnr", "ssim", "mae"):
        assert torch.equal(ev_result[k + "_per_sample"], pm[k].view(Mt, S)), k
        assert ev_result[k] == float(pm[k].mean()), k


def evaluator_in_any_arrival_order(dev):
    """Random images in a shuffled arrival order; the last condition has no target (diversity only); reading early raises."""
    import pytest
    from bbdm_amd import metrics
    M, S = 4, 3
    samples = _rand_u8((M, S, 13, 19, 3), 3).to(dev)
    targets = _rand_u8((M - 1, 13, 19, 3), 4).to(dev)
    ev = metrics.SetEvaluator(S)
    with pytest.raises(ValueError):
        ev.result()
    order = [(m, s) for m in range(M) for s in range(S)]
    perm = torch.randperm(len(order), generator=torch.Generator().manual_seed(9)).tolist()
    for m in reversed(range(M - 1)):
        ev.add_target(m, targets[m])
    for i in perm[:-1]:
        ev.add_sample(*order[i], samples[order[i]])
    with pytest.raises(ValueError, match="have not arrived"):
        ev.result()
    with pytest.raises(ValueError):
        ev.add_sample(0, S, samples[0, 0])
    ev.consume([(order[perm[-1]], samples[order[perm[-1]]])])
    r = ev.result()
    assert sorted(r["conditions"]) == list(range(M)) and sorted(r["paired_conditions"]) == list(range(M - 1))
    idx = torch.tensor(r["conditions"])
    assert r["paired_conditions"] == [m for m in r["conditions"] if m < M - 1]
    pidx = torch.tensor(r["paired_conditions"])
    # per-item arrays follow the order of first arrival: compare per key
    per, _ = metrics.diversity(samples)
    assert torch.equal(r["diversity_per_condition"], per[idx])
    pm = metrics.pair_metrics(samples[:M - 1].flatten(0, 1), targets.repeat_interleave(S, 0))
    for k in ("psnr", "ssim", "mae"):
        assert torch.equal(r[k + "_per_sample"], pm[k].view(M - 1, S)[pidx]), k
    # the means do not depend on the order beyond fp64 summation: recompute them in the evaluator's order
    assert r["diversity"] == float(per[idx].mean())
    assert r["ssim"] == float(pm["ssim"].view(M - 1, S)[pidx].flatten().mean())


def evaluator_consumes_a_sampler(dev):
    """A tiny BridgeSampler run (the golden tiny_concat UNet, 6-step schedule): ``consume`` of the sampler's iterator equals the
    metrics of the tensor ``sample_set`` returns for the same seeds."""
    import sampler_cases as SC
    from bbdm_amd import BridgeSampler, egress, metrics
    m, _ = SC.tiny_concat(dev, 6)
    M, S = 3, 2
    g = torch.Generator().manual_seed(31)
    conds = torch.randn(M, 3, 16, 16, generator=g).clamp(-1, 1).to(dev)
    gts = torch.randn(M, 3, 16, 16, generator=g).clamp(-1, 1).to(dev)
    seeds = [500 + k for k in range(M * S)]
    s = BridgeSampler(m, 4, noise="philox")
    s.submit([((mi, j), conds[mi], seeds[mi * S + j]) for mi in range(M) for j in range(S)])
    ev = metrics.SetEvaluator(S)
    for mi in range(M):
        ev.add_target(mi, gts[mi])
    r = ev.consume(s).result()
    assert r["conditions"] and sorted(r["conditions"]) == [0, 1, 2]
    out = BridgeSampler(m, 4, noise="philox").sample_set(conds, S, seeds)            # [M, S, C, H, W], the same samples
    order = torch.tensor(r["conditions"], device=dev)
    su8 = egress._to_u8_device(out.flatten(0, 1), True).view(M, S, 16, 16, 3)[order]
    tu8 = egress._to_u8_device(gts, True)[order]
    _check_against_assembled(r, su8, tu8, S)
    assert math.isfinite(r["psnr"]) and -1.0 <= r["ssim"] <= 1.0 and r["diversity"] >= 0.0
