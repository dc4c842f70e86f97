#!/usr/bin/env python
"""A/B of the LBBDM-f4 training micro-step (forward + backward) through ``forward(images)`` and through ``forward(indices)`` on an
attached latent cache, in one process on one MI355X; plus the cache's build throughput and the ``mean_std()`` time.

    python tools/latent_cache_bench.py [--batch 32] [--pairs 128] [--reps 10] [--rounds 3] [--stats-rows 4096] > profiles/latent_cache.txt

Shapes: the LBBDM-f4 template (bench.py's c4 UNet and c3 first stage: 256x256 images -> 3x64x64 latents), random-init weights (the
time does not depend on the values).  Timing: device events around ``reps`` micro-steps after a warm-up of every shape, the two paths
alternating over ``rounds`` so that drift of the shared host shows as spread rather than as a difference.  Before any timing the two
paths are compared on the same batch from the same generator state (loss and one gradient, bitwise), and torch's fp32 division on the
device is compared with a float64 evaluation (the bitwise kernel tests rest on it being correctly rounded)."""
import argparse
import os
import sys
import time

import torch
from torch.utils.data import Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the template shapes live there)
import bbdm_amd  # noqa: E402
from bbdm_amd.latent_cache import LatentCache, channel_stats  # noqa: E402


class Pairs(Dataset):
    def __init__(self, n, size):
        g = torch.Generator().manual_seed(3)
        self.x = torch.randn(n, 3, size, size, generator=g).clamp(-1, 1)
        self.c = torch.randn(n, 3, size, size, generator=g).clamp(-1, 1)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return (self.x[i], f"{i:06d}"), (self.c[i], f"{i:06d}")


def timed(fn, reps, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / reps


def division_check(dev):
    g = torch.Generator().manual_seed(1)
    a = (torch.randn(1 << 20, generator=g) * 3).to(dev)
    b = (torch.rand(1 << 20, generator=g) * 3.5 + 0.5).to(dev)
    q = a / b
    exact = (a.double() / b.double()).float()          # fp64 quotient of fp32 operands rounds to the correctly rounded fp32 quotient
    return int((q != exact).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stats-rows", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latent_cache_bench: needs the GPU (no CPU timing is meaningful)")
    dev = torch.device("cuda:0")
    _, unet, _, _, _, _, _ = bench.WORKLOADS["c4"]
    cfg = bench._ns({"BB": {"params": dict(bench.BB, skip_sample=True, sample_step=200, UNetParams=unet)},
                     "VQGAN": {"params": dict(bench.FIRST_STAGE["c3"], ckpt_path=None, lossconfig={"target": "torch.nn.Identity"})},
                     "normalize_latent": True, "latent_before_quant_conv": False})
    torch.manual_seed(7)
    m = bbdm_amd.LatentBrownianBridgeModel(cfg).to(dev).train()
    ds = Pairs(args.pairs, 256)
    print(f"# latent cache A/B, LBBDM-f4 template shapes, batch {args.batch}, {torch.cuda.get_device_name(dev)}")
    print(f"torch fp32 division on the device vs the rounded float64 quotient, 2^20 pairs: {division_check(dev)} mismatches")

    LatentCache.build(m, ds, batch_size=args.batch)                      # warm-up of the encoder plan
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    cache = LatentCache.build(m, ds, batch_size=args.batch)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    print(f"build: {args.pairs} pairs of 256x256 in {dt * 1e3:.1f} ms = {args.pairs / dt:.1f} pairs/s = {2 * args.pairs / dt:.1f} images/s "
          f"(host clock around a synchronise; in-memory dataset, verify=8); rows {tuple(cache.ori.shape)}")
    cache.install_stats(m)
    m.attach_latent_cache(cache)

    x, c = ds.x[:args.batch].to(dev), ds.c[:args.batch].to(dev)
    idx = torch.arange(args.batch, dtype=torch.int64, device=dev)

    def step(a, b):
        for p in m.denoise_fn.parameters():
            p.grad = None
        loss, _ = m(a, b)
        loss.backward()
        return loss

    probe = next(m.denoise_fn.parameters())
    res = []
    for a, b in ((x, c), (idx, idx)):
        torch.manual_seed(11)
        loss = step(a, b)
        res.append((loss.detach().clone(), probe.grad.clone()))
    same = torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    print(f"same generator state, images vs indices: loss {float(res[0][0]):.8f} / {float(res[1][0]):.8f}, loss and first-parameter "
          f"gradient bitwise equal: {same}")
    for a, b in ((x, c), (idx, idx)):                                    # warm-up of both paths
        for _ in range(2):
            step(a, b)
    img, ind = [], []
    for _ in range(args.rounds):
        img.append(timed(lambda: step(x, c), args.reps, dev))
        ind.append(timed(lambda: step(idx, idx), args.reps, dev))
    print(f"micro-step (forward + backward), ms per step over {args.reps} steps, {args.rounds} alternating rounds (device events):")
    print("  forward(images):  " + "  ".join(f"{v:.2f}" for v in img) + f"   median {sorted(img)[len(img) // 2]:.2f}")
    print("  forward(indices): " + "  ".join(f"{v:.2f}" for v in ind) + f"   median {sorted(ind)[len(ind) // 2]:.2f}")
    enc = timed(lambda: (m.encode(x, cond=False), m.encode(c, cond=True)), args.reps, dev)
    print(f"  the two encodes of the image path alone: {enc:.2f} ms")

    # what the index path adds to a UNet micro-step that starts from latents: the gather kernel in place of q_sample
    lat_o, lat_c = cache.ori[:args.batch].clone(), cache.cond[:args.batch].clone()
    t = torch.randint(0, 1000, (args.batch,), device=dev)
    q_plain = timed(lambda: m.q_sample((lat_o - m.ori_latent_mean) / m.ori_latent_std, (lat_c - m.cond_latent_mean) / m.cond_latent_std,
                                       t, torch.randn_like(lat_o)), 200, dev)
    m.model_config.normalize_latent = False
    q_raw = timed(lambda: m.q_sample(lat_o, lat_c, t, torch.randn_like(lat_o)), 200, dev)
    m.model_config.normalize_latent = True

    def cached_q():
        orig = m._denoise_and_loss
        m._denoise_and_loss = lambda *a: None
        try:
            m.p_losses_cached(idx, idx, t)
        finally:
            m._denoise_and_loss = orig
    q_cached = timed(cached_q, 200, dev)
    print(f"q_sample alone, ms per call over 200 calls (randn included): on latents {q_raw:.4f}; torch normalise + q_sample {q_plain:.4f}; "
          f"gather + normalise + q_sample from the cache {q_cached:.4f}")

    rows = args.stats_rows
    z = torch.randn(rows, 3, 64, 64, device=dev) * 2 + 5
    channel_stats(z)
    st = timed(lambda: channel_stats(z), 5, dev)
    gb = z.numel() * 4 * 2 / 1e9
    print(f"channel statistics of one [{rows}, 3, 64, 64] tensor (two passes, {gb:.2f} GB read): {st:.3f} ms = {gb / (st * 1e-3):.0f} GB/s; "
          f"mean_std() runs it on both tensors: {2 * st:.3f} ms")


if __name__ == "__main__":
    main()
