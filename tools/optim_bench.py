#!/usr/bin/env python
"""Time of one optimizer step at the full-size UNet's parameter count (bench.WORKLOADS["c4"]: 248 tensors, 237 M parameters) for
every optimizer the training config can select (runners/utils.py:48-57), fused (bbdm_amd.optim) and torch's own, in ONE process:

  FusedSGD(momentum=0.9) / FusedRMSprop() / FusedAdam()      each plain, clipped (max_grad_norm=1, skip_nonfinite) and with the
                                                             EMA update fused into the pass (step(ema=...))
  torch.optim.SGD(momentum=0.9) / torch.optim.RMSprop()      step alone, + a separate EMA.update (bbdm_amd's one-launch EMA), +
                                                             torch.nn.utils.clip_grad_norm_ in front, and all three: what
                                                             get_optimizer's 'SGD' / 'RMSProp' ran before they had a fused step

Every configuration owns its parameters, gradients (randn * 1e-3: global norm 15.4, so max_grad_norm = 1 clips) and state.  A window
is ``--launches`` steps between two device events; the configurations take turns window by window (``--windows`` rounds), so drift
of the machine lands on all of them alike.  Reported per configuration: the median window, the fastest and the slowest (ms per step),
and the bytes the rule has to move (4 B x parameters x tensors read or written) over the median time.

    python tools/optim_bench.py [--launches 200] [--windows 5] [--out profiles/optim_rules.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--only", default=None, help="comma-separated substrings: time only the configurations whose name has one")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    import bbdm_amd
    from bbdm_amd.optim import EMA, FusedAdam, FusedRMSprop, FusedSGD

    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py times the GPU: no device found")
    dev = torch.device("cuda:0")
    shapes = [tuple(p.shape) for p in bbdm_amd.unet.UNetModel(**bench.WORKLOADS["c4"][1]).parameters()]
    count = sum(torch.Size(s).numel() for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(3)
    lr = 1e-6                                         # small: thousands of steps on random gradients keep the weights finite

    def fresh():
        holder = nn.Module()
        holder.ps = nn.ParameterList([nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02) for s in shapes])
        for p in holder.ps:
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
        return holder

    def with_ema(holder):
        ema = EMA(0.995)
        ema.register(holder)
        return ema

    configs = []                                      # (name, tensors moved per parameter, step function)

    def fused(name, make, moved):
        h = fresh()
        opt = make(h.parameters(), {})
        configs.append((f"{name}", moved, opt.step))
        h = fresh()
        opt = make(h.parameters(), dict(max_grad_norm=1.0, skip_nonfinite=True))
        configs.append((f"{name} clipped", moved + 1, opt.step))
        h = fresh()
        opt, ema = make(h.parameters(), {}), with_ema(h)
        configs.append((f"{name} + fused EMA", moved + 2, lambda opt=opt, ema=ema: opt.step(ema=ema, ema_with_decay=True)))

    def torchs(name, make, moved):
        h = fresh()
        opt = make(h.parameters())
        configs.append((f"{name}", moved, opt.step))
        h = fresh()
        opt, ema = make(h.parameters()), with_ema(h)

        def step_ema(opt=opt, ema=ema, h=h):
            opt.step()
            ema.update(h)
        configs.append((f"{name}, EMA.update", moved + 3, step_ema))
        h = fresh()
        opt, ps = make(h.parameters()), list(h.parameters())

        def clip_step(opt=opt, ps=ps):
            torch.nn.utils.clip_grad_norm_(ps, 1.0)
            opt.step()
        configs.append((f"clip_grad_norm_, {name}", moved + 3, clip_step))
        h = fresh()
        opt, ps, ema = make(h.parameters()), list(h.parameters()), with_ema(h)

        def clip_step_ema(opt=opt, ps=ps, ema=ema, h=h):
            torch.nn.utils.clip_grad_norm_(ps, 1.0)
            opt.step()
            ema.update(h)
        configs.append((f"clip_grad_norm_, {name}, EMA.update", moved + 6, clip_step_ema))

    # tensors moved per parameter by the rule alone: SGD p, g, buf read + p, buf written; RMSprop p, g, sq + p, sq; Adam p, g, m, v +
    # p, m, v.  Clipping reads g once more; a fused EMA reads and writes the shadow; a separate EMA.update reads p as well; torch's
    # clip reads g, then reads and writes it.  (What torch's foreach steps really move is more: they make several passes.)
    fused("FusedSGD(momentum=0.9)", lambda ps, kw: FusedSGD(ps, lr=lr, momentum=0.9, **kw), 5)
    fused("FusedRMSprop()", lambda ps, kw: FusedRMSprop(ps, lr=lr, **kw), 5)
    fused("FusedAdam()", lambda ps, kw: FusedAdam(ps, lr=lr, **kw), 7)
    torchs("torch.optim.SGD(momentum=0.9)", lambda ps: torch.optim.SGD(ps, lr=lr, momentum=0.9), 5)
    torchs("torch.optim.RMSprop()", lambda ps: torch.optim.RMSprop(ps, lr=lr), 5)
    if args.only:
        keys = args.only.split(",")
        configs = [c for c in configs if any(k in c[0] for k in keys)]

    for _, _, fn in configs:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in configs}
    for w in range(args.windows):
        for name, _, fn in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.launches)
        print(f"window {w + 1}/{args.windows} done", flush=True)

    lines = [f"{count / 1e6:.1f} M parameters in {len(shapes)} tensors; {args.windows} windows of {args.launches} steps per configuration, "
             f"taken in turns; torch {torch.__version__}, {torch.cuda.get_device_name(0)}",
             f"{'configuration':<62} {'median':>8} {'fastest':>8} {'slowest':>8}  ms/step   spread   least bytes   at the median"]
    for name, moved, _ in configs:
        t = times[name]
        med = statistics.median(t)
        gb = 4 * count * moved / 1e9
        lines.append(f"{name:<62} {med:8.3f} {min(t):8.3f} {max(t):8.3f}            {100 * (max(t) - min(t)) / med:5.1f} %   {gb:6.2f} GB   "
                     f"{gb / med:6.2f} TB/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
