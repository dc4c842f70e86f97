#!/usr/bin/env python
"""Throughput of a MIX of sampling schedules on the C3 configuration of tools/bench_sampler.py (LBBDM-f4 UNet, latent 3x64x64, HIP first
stage at 256^2): ``--conds`` conditions x ``--sample-num`` samples, the samples of even conditions at ``--short`` steps (a preview), of
odd conditions at ``--long`` steps (a final).

  --mode mixed : ONE ``BridgeSampler(model, --width)`` takes all requests, each with its ``SamplingParams(sample_step=...)``.
  --mode split : what a checkout without per-request parameters can do -- two models of the same weights, one per ``sample_step``,
                 each with its own width ``--width`` sampler, run one after the other.  With ``--root`` naming another checkout (the
                 parent commit) its ``bbdm_amd`` and ``bench.py`` are imported instead.

One untimed pass (``--warmup``) builds the plans and graphs; then ``--reps`` timed passes over the whole set, each ended by a device
synchronisation.  Prints one JSON line: images per second of every repetition, and the sampler steps of one pass."""
import argparse
import json
import os
import sys
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("mixed", "split"), required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--conds", type=int, default=20)
    ap.add_argument("--sample-num", type=int, default=5)
    ap.add_argument("--short", type=int, default=20)
    ap.add_argument("--long", type=int, default=200)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import bench                                   # the C3 geometry and the synthetic UNet weights of bench.py
    import bbdm_amd

    dev = torch.device("cuda:0")
    _, up, ch, size, _, skip, _ = bench.WORKLOADS["c3"]
    fs = dict(bench.FIRST_STAGE["c3"], ckpt_path=None, lossconfig={"target": "torch.nn.Identity"})

    def build(sample_step):
        cfg = bench._ns({"BB": {"params": dict(bench.BB, skip_sample=True, sample_step=sample_step, UNetParams=up)},
                         "VQGAN": {"params": fs}, "normalize_latent": False, "latent_before_quant_conv": False})
        torch.manual_seed(7)
        model = bbdm_amd.LatentBrownianBridgeModel(cfg)
        model.denoise_fn.load_state_dict(bench.synth_state(model.denoise_fn), strict=True)
        return model.to(dev).eval()

    g = torch.Generator().manual_seed(1234)
    res = fs["ddconfig"]["resolution"]
    conds = torch.randn(args.conds, 3, res, res, generator=g).clamp(-1, 1).to(dev)
    n_img = args.conds * args.sample_num
    seeds = list(range(n_img))
    steps = [0]

    def gen(seed):
        gg = torch.Generator(device=dev)
        gg.manual_seed(seed)
        return gg

    def drain(sampler, out):
        while sampler.busy():
            for key, img in sampler.step():
                out[key] = img
            steps[0] += 1

    if args.mode == "mixed":
        sampler = bbdm_amd.BridgeSampler(build(args.long), args.width)
        params = [bbdm_amd.SamplingParams(sample_step=args.short), bbdm_amd.SamplingParams(sample_step=args.long)]

        def one_pass():
            out = {}
            for b0 in range(0, args.conds, args.group):
                sampler.submit([((m, s), conds[m], gen(seeds[m * args.sample_num + s]), params[m % 2])
                                for m in range(b0, min(args.conds, b0 + args.group)) for s in range(args.sample_num)])
            drain(sampler, out)
            return out
    else:
        samplers = [bbdm_amd.BridgeSampler(build(args.short), args.width), bbdm_amd.BridgeSampler(build(args.long), args.width)]

        def one_pass():
            out = {}
            for which, sampler in enumerate(samplers):
                for b0 in range(0, args.conds, args.group):
                    reqs = [((m, s), conds[m], gen(seeds[m * args.sample_num + s]))
                            for m in range(b0, min(args.conds, b0 + args.group)) if m % 2 == which for s in range(args.sample_num)]
                    sampler.submit(reqs)
                drain(sampler, out)
            return out

    with torch.no_grad():
        for _ in range(args.warmup):
            one_pass()
        torch.cuda.synchronize(dev)
        times = []
        for _ in range(args.reps):
            steps[0] = 0
            t0 = time.perf_counter()
            out = one_pass()
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
            assert len(out) == n_img
            del out
    print(json.dumps({"mode": args.mode, "width": args.width, "package": bbdm_amd.__file__, "images": n_img,
                      "schedules": [args.short, args.long], "sampler_steps_per_pass": steps[0],
                      "seconds": [round(t, 3) for t in times], "imgs_per_s": [round(n_img / t, 3) for t in times]}), flush=True)


if __name__ == "__main__":
    main()
