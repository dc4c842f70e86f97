#!/usr/bin/env python
"""Throughput of the reference's evaluation pattern (BBDMRunner.sample_to_eval, runners/DiffusionBasedModelRunners/BBDMRunner.py:224-253)
on the C3 configuration: LBBDM-f4 UNet (latent 3x64x64, 200 steps), the HIP first stage at 256^2, ``--conds`` conditions x
``--sample-num`` samples.

  --mode baseline : ``net.sample(x_cond)`` ``sample_num`` times per test batch of ``--group`` (8), the reference's loop.  With
                    ``--root`` naming another checkout (the parent commit) its ``bbdm_amd`` and ``bench.py`` are imported instead.
  --mode sampler  : ``BridgeSampler(model, --width).sample_set(conds, sample_num, seeds)`` (bbdm_amd/sampler.py).  ``--noise philox``:
                    the sampler's seed-addressed noise, generated inside the bridge launch (no ``normal_`` launches); ``torch`` (the
                    default) also runs against a ``--root`` checkout that predates the option.

One untimed pass (``--warmup``) builds the plans and graphs; then ``--reps`` timed passes over the whole set, each ended by a device
synchronisation.  Prints one JSON line: images per second of every repetition."""
import argparse
import json
import os
import sys
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("baseline", "sampler"), required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--conds", type=int, default=20)
    ap.add_argument("--sample-num", type=int, default=5)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--noise", choices=("torch", "philox"), default="torch")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import bench                                   # the C3 geometry and the synthetic UNet weights of bench.py
    import bbdm_amd

    dev = torch.device("cuda:0")
    _, up, ch, size, _, skip, sstep = bench.WORKLOADS["c3"]
    fs = dict(bench.FIRST_STAGE["c3"], ckpt_path=None, lossconfig={"target": "torch.nn.Identity"})
    cfg = bench._ns({"BB": {"params": dict(bench.BB, skip_sample=skip, sample_step=sstep, UNetParams=up)},
                     "VQGAN": {"params": fs}, "normalize_latent": False, "latent_before_quant_conv": False})
    torch.manual_seed(7)
    model = bbdm_amd.LatentBrownianBridgeModel(cfg)
    model.denoise_fn.load_state_dict(bench.synth_state(model.denoise_fn), strict=True)
    model = model.to(dev).eval()
    g = torch.Generator().manual_seed(1234)
    res = fs["ddconfig"]["resolution"]
    conds = torch.randn(args.conds, 3, res, res, generator=g).clamp(-1, 1).to(dev)
    n_img = args.conds * args.sample_num

    if args.mode == "baseline":
        def one_pass():
            outs = []
            for b0 in range(0, args.conds, args.group):
                x_cond = conds[b0:b0 + args.group]
                for _ in range(args.sample_num):
                    outs.append(model.sample(x_cond))
            return outs
    else:
        sampler = bbdm_amd.BridgeSampler(model, args.width, **({"noise": "philox"} if args.noise == "philox" else {}))
        seeds = list(range(n_img))

        def one_pass():
            return sampler.sample_set(conds, args.sample_num, seeds, group=args.group)

    with torch.no_grad():
        for _ in range(args.warmup):
            one_pass()
        torch.cuda.synchronize(dev)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = one_pass()
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
            del out
    line = {"mode": args.mode, "noise": args.noise if args.mode == "sampler" else "torch", "width": args.width if args.mode == "sampler" else args.group, "package": bbdm_amd.__file__,
            "images": n_img, "steps": len(model.steps), "seconds": [round(t, 3) for t in times],
            "imgs_per_s": [round(n_img / t, 3) for t in times]}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
