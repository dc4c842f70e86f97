#!/usr/bin/env python
"""Scoring a sample set on the device against the file route (bbdm_amd/metrics.py), on one MI355X.

At C3's evaluation pattern (``--conds`` 20 conditions x ``--sample-num`` 5 samples) with 3 x 64 x 64 and with 3 x 256 x 256 images:

  device   : ``SetEvaluator`` fed the fp32 device tensors one image at a time (``add_target`` / ``add_sample``), then ``result()``;
             and the batch calls ``diversity`` + ``pair_metrics`` on the assembled tensors alone;
  files    : ``metrics_from_dirs`` over the PNG files ``ImageWriter`` wrote in ``sample_to_eval``'s layout (decode + upload + the
             same kernels);
  cpu loop : a plain restatement of the reference's ``calc_diversity`` loop (evaluation/diversity.py:8-39: every file opened with
             PIL, ``ToTensor() * 255`` as ``uint8 -> float / 255 * 255``, the fp32 mean / variance / root with torch on the CPU).

Times are host clocks around a device synchronisation (every route ends on the host), median of ``--reps`` runs after one warm-up.
The values of the routes are compared as well: files vs tensors must be equal, the CPU loop differs by its fp32 ``torch.mean``.
Writes its lines to ``--out`` (default profiles/metrics.txt)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_diversity_loop(result_dir, names, num_samples):
    import numpy as np
    from PIL import Image
    std = 0
    for name in names:
        imgs = []
        for j in range(num_samples):
            img = Image.open(os.path.join(result_dir, name, f"output_{j}.png")).convert("RGB")
            t = torch.from_numpy(np.array(img)).permute(2, 0, 1).to(torch.float32).div(255)          # ToTensor()
            imgs.append(t * 255.)
        mean = torch.zeros_like(imgs[0])
        for j in range(num_samples):
            mean = mean + imgs[j]
        mean = mean / num_samples
        var = torch.zeros_like(imgs[0])
        for j in range(num_samples):
            var = var + (imgs[j] - mean) ** 2
        var = var / num_samples
        std = std + torch.mean(torch.sqrt(var))
    return float(std / len(names))


def timed(fn, reps, sync):
    fn()
    out, ts = None, []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def fmt(ts):
    return "  ".join(f"{t:.2f}" for t in ts) + f"   median {statistics.median(ts):.2f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conds", type=int, default=20)
    ap.add_argument("--sample-num", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics.txt"))
    args = ap.parse_args()
    from bbdm_amd import egress, metrics

    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    M, S = args.conds, args.sample_num
    lines = [f"# evaluation metrics, {M} conditions x {S} samples, {torch.cuda.get_device_name(0)}; host clock, ms, {args.reps} runs after a warm-up"]
    for size in args.sizes:
        g = torch.Generator().manual_seed(size)
        gts = torch.randn(M, 3, size, size, generator=g).mul(0.5).clamp(-1, 1)
        samples = (gts[:, None] + 0.25 * torch.randn(M, S, 3, size, size, generator=g)).clamp(-1, 1).to(dev)
        gts = gts.to(dev)

        def evaluator():
            ev = metrics.SetEvaluator(S)
            for m in range(M):
                ev.add_target(m, gts[m])
                for j in range(S):
                    ev.add_sample(m, j, samples[m, j])
            return ev.result()

        def batch_calls():
            d = metrics.diversity(samples)
            p = metrics.pair_metrics(samples[:, :, :].flatten(0, 1), gts.repeat_interleave(S, 0))
            return d, p

        r_dev, t_dev = timed(evaluator, args.reps, sync)
        _, t_batch = timed(batch_calls, args.reps, sync)
        with tempfile.TemporaryDirectory() as tmp:
            res, gt = os.path.join(tmp, "200"), os.path.join(tmp, "ground_truth")
            os.makedirs(gt)
            names = [str(m) for m in range(M)]
            t0 = time.perf_counter()
            with egress.ImageWriter() as w:
                for m in range(M):
                    os.makedirs(os.path.join(res, names[m]))
                    w.submit(samples[m], os.path.join(res, names[m]), [f"output_{j}.png" for j in range(S)])
                w.submit(gts, gt, [n + ".png" for n in names])
            t_write = (time.perf_counter() - t0) * 1e3
            order = sorted(names)
            r_files, t_files = timed(lambda: metrics.metrics_from_dirs(res, gt, S, device=dev), args.reps, sync)
            d_cpu, t_cpu = timed(lambda: cpu_diversity_loop(res, order, S), args.reps, lambda: None)
        # metrics_from_dirs takes the conditions in sorted name order ("0", "1", "10", ...): compare per condition
        perm = [int(n) for n in r_files["conditions"]]
        same = all(float(r_files["diversity_per_condition"][i]) == float(r_dev["diversity_per_condition"][m]) and
                   torch.equal(r_files["ssim_per_sample"][i], r_dev["ssim_per_sample"][m]) and
                   torch.equal(r_files["mse_per_sample"][i], r_dev["mse_per_sample"][m]) for i, m in enumerate(perm))
        lines += [
            f"## {M} x {S} images of 3 x {size} x {size}",
            f"device, SetEvaluator (add_target / add_sample per image + result): {fmt(t_dev)}",
            f"device, diversity + pair_metrics on the assembled tensors:          {fmt(t_batch)}",
            f"files,  metrics_from_dirs (decode {M * (S + 1)} PNGs + upload + kernels):   {fmt(t_files)}   (writing them: {t_write:.1f} ms once)",
            f"cpu,    the reference's diversity loop on the files (diversity only): {fmt(t_cpu)}",
            f"values: diversity {r_dev['diversity']!r} psnr {r_dev['psnr']!r} ssim {r_dev['ssim']!r} mae {r_dev['mae']!r}",
            f"        files == tensors per condition and sample (diversity, ssim, mse): {same}",
            f"        reference loop (fp32 torch.mean, torch's CPU sqrt) {d_cpu!r}: relative difference {abs(d_cpu - r_dev['diversity']) / r_dev['diversity']:.2e}",
        ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
