#!/usr/bin/env python
"""Cost of the loss meter (bbdm_amd/loss_meter.py) on the LBBDM-f4 training micro-step, on one MI355X.

    python tools/loss_meter_bench.py [--steps 20] [--rounds 5] [--reps 200] [--tree DIR] [--label NAME] >> profiles/loss_meter.txt

The micro-step is bench.py's c4: its UNet, its inputs ([32, 3, 64, 64] latents), ``net(x, y)`` -> ``loss.backward()`` and the fused
Adam step on every 4th micro-step, timed with device events over ``steps`` micro-steps after a primed accumulation cycle and a warm-up.
Rounds alternate between no meter and an attached ``train`` meter, so that drift of a shared host shows as spread within a column and not
as a difference between the columns.  Then the meter's launches alone (``LossMeter.add`` on the same shapes, ``reps`` calls between
two events) and ``read()``.

``--tree DIR`` imports bench.py and bbdm_amd from another checkout (built there) -- the parent commit, whose micro-step is the baseline
the detached column has to equal; a tree without ``bbdm_amd.LossMeter`` runs the detached column only."""
import argparse
import os
import sys

import torch


def timed(fn, reps, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / reps


def row(name, vals):
    s = sorted(vals)
    return f"  {name:<28}" + "  ".join(f"{v:.3f}" for v in vals) + f"   median {s[len(s) // 2]:.3f}  min {s[0]:.3f}  max {s[-1]:.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_meter_bench: needs the GPU (no CPU timing is meaningful)")
    sys.path.insert(0, os.path.abspath(args.tree))
    import bench
    import bbdm_amd
    from bbdm_amd import _lib
    from bbdm_amd.optim import FusedAdam
    dev = torch.device("cuda:0")
    _, up, ch, size, batch, skip, sstep = bench.WORKLOADS["c4"]
    model = bbdm_amd.BrownianBridgeModel(bench._ns({"BB": {"params": dict(bench.BB, skip_sample=skip, sample_step=sstep, UNetParams=up)}}))
    model.denoise_fn.load_state_dict(bench.synth_state(model.denoise_fn), strict=True)
    model = model.to(dev).train()
    x, y = (v.to(dev) for v in bench.make_inputs(batch, ch, size, seed=1234))
    torch.manual_seed(1234)
    opt = FusedAdam(model.get_parameters(), lr=1e-4, betas=(0.9, 0.999))
    accumulate = 4
    has_meter = hasattr(bbdm_amd, "LossMeter")
    print(f"# {args.label}: ABI {_lib.load().bbdm_version()}, LossMeter {'present' if has_meter else 'absent'}; c4 micro-step, batch {batch}, "
          f"latent {ch}x{size}x{size}, {torch.cuda.get_device_name(dev)}")

    def step(i):
        loss, _ = model(x, y)
        loss.backward()
        if (i + 1) % accumulate == 0:
            opt.step()
            opt.zero_grad(set_to_none=True)

    for i in range(accumulate + 4):                                     # the first optimizer step allocates the moments
        step(i)
    meter = bbdm_amd.LossMeter(model.num_timesteps, 10, device=dev, loss_type=model.loss_type) if has_meter else None
    if has_meter:
        model.attach_loss_meter(train=meter)
        for i in range(accumulate):
            step(i)
        model.detach_loss_meter()
    off, on = [], []
    for _ in range(args.rounds):
        off.append(timed(step, args.steps, dev))
        if has_meter:
            model.attach_loss_meter(train=meter)
            on.append(timed(step, args.steps, dev))
            model.detach_loss_meter()
    print(f"micro-step (forward + backward, fused Adam on every {accumulate}th), ms per step over {args.steps} steps, {args.rounds} "
          f"alternating rounds (device events):")
    print(row("no meter attached:", off))
    if not has_meter:
        return
    print(row("train meter attached:", on))
    r = meter.read()
    print(f"  the meter after those rounds: {int(r['count'].sum())} images, loss {r['loss']:.6f}, rejected {r['rejected']}, "
          f"count per bucket {r['count'].tolist()}")
    meter.reset()
    g = torch.Generator().manual_seed(5)
    a, b = (torch.randn(batch, ch, size, size, generator=g).to(dev) for _ in range(2))
    t = torch.randint(0, model.num_timesteps, (batch,), generator=g).to(dev)
    for _ in range(20):
        meter.add(a, b, t)
    adds = [timed(lambda i: meter.add(a, b, t), args.reps, dev) for _ in range(3)]
    print(f"LossMeter.add alone on [{batch}, {ch}, {size}, {size}] (zero the cells, per-image pass, accumulate), ms per call over "
          f"{args.reps} back-to-back calls, 3 runs (device events; host-bound when the launches are shorter than their issue):")
    print(row("add:", adds))
    meter.reset()
    for _ in range(100):
        meter.add(a, b, t)
    reads = [timed(lambda i: meter.read(), 20, dev) for _ in range(3)]
    print(row("read (syncs), ms:", reads))


if __name__ == "__main__":
    main()
