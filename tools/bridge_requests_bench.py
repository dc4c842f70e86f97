#!/usr/bin/env python
"""Kernel cost of the per-request bridge entry points (bbdm_bb_p_sample_step_requests_f32 / _requests_philox_f32) against the
uniform ones (bbdm_bb_p_sample_step_batched_f32 / _philox_f32), with uniform parameters, on the two shapes the sampler and the
benchmark use: C3's sampler (width 32, 3x64x64 latents) and C2 (16 x 3x256x256).

``--parent-lib PATH`` names a libbbdm_hip.so built from the parent commit: its uniform entry points are timed in the same process,
alternating with this build's.  Each figure is the mean over ``--launches`` back-to-back launches between two device events, after a
warm-up; ``--reps`` such windows per entry point, interleaved.  Prints one JSON line per (shape, entry point): microseconds per launch
of every window."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = ctypes.c_void_p
UNIFORM = [P] * 9 + [ctypes.c_float, ctypes.c_int, ctypes.c_int] + [P] * 3 + [ctypes.c_int, ctypes.c_int, P]
UNIFORM_PHILOX = [P] * 10 + [ctypes.c_float, ctypes.c_int, ctypes.c_int] + [P] * 3 + [ctypes.c_int, ctypes.c_int, P]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    from bbdm_amd import _lib, bridge_schedule
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    tables, _ = bridge_schedule(1000, "linear", 1.0, True, "linear", 200)
    m_t = torch.tensor(tables["m_t"], dtype=torch.float32, device=dev)
    var_t = torch.tensor(tables["variance_t"], dtype=torch.float32, device=dev)
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name, sig in (("bbdm_bb_p_sample_step_batched_f32", UNIFORM), ("bbdm_bb_p_sample_step_philox_f32", UNIFORM_PHILOX)):
            getattr(parent, name).restype, getattr(parent, name).argtypes = ctypes.c_int, sig

    for label, shape in (("c3_sampler_32x3x64x64", (32, 3, 64, 64)), ("c2_16x3x256x256", (16, 3, 256, 256))):
        N, per = shape[0], shape[1] * shape[2] * shape[3]
        g = torch.Generator(device=dev).manual_seed(1)
        x, y, pred, noise = (torch.randn(shape, generator=g, device=dev) for _ in range(4))
        xn, x0, alias = (torch.empty(shape, device=dev) for _ in range(3))
        steps = [int(s) for s in torch.linspace(999, 5, N)]
        t = torch.tensor(steps, dtype=torch.int64, device=dev)
        tn = t - 5
        state = torch.zeros(N, dtype=torch.int64, device=dev)
        flag = state | 4
        eta = torch.ones(N, dtype=torch.float32, device=dev)
        seed = torch.arange(N, dtype=torch.int64, device=dev) + 100
        ordinal = torch.arange(N, dtype=torch.int64, device=dev)
        p = lambda a: a.data_ptr()
        head = (p(x), p(y), p(pred))
        tabs = (p(m_t), p(var_t), p(t), p(tn))
        tail = (0, p(xn), p(x0), p(alias), N, per, stream)
        runs = {
            "batched": lambda: lib.bbdm_bb_p_sample_step_batched_f32(*head, p(noise), *tabs, p(state), 1.0, 1, *tail),
            "requests": lambda: lib.bbdm_bb_p_sample_step_requests_f32(*head, p(noise), *tabs, p(flag), p(eta), *tail),
            "philox": lambda: lib.bbdm_bb_p_sample_step_philox_f32(*head, p(seed), p(ordinal), *tabs, p(state), 1.0, 1, *tail),
            "requests_philox": lambda: lib.bbdm_bb_p_sample_step_requests_philox_f32(*head, p(seed), p(ordinal), *tabs, p(flag),
                                                                                      p(eta), *tail),
        }
        if parent is not None:
            runs["parent_batched"] = lambda: parent.bbdm_bb_p_sample_step_batched_f32(*head, p(noise), *tabs, p(state), 1.0, 1, *tail)
            runs["parent_philox"] = lambda: parent.bbdm_bb_p_sample_step_philox_f32(*head, p(seed), p(ordinal), *tabs, p(state), 1.0,
                                                                                    1, *tail)
        outs = {}
        for name, fn in runs.items():                       # warm-up, and the results of the timed shapes for the equality check
            for _ in range(20):
                assert fn() == 0, name
            torch.cuda.synchronize(dev)
            outs[name] = (xn.clone(), x0.clone(), alias.clone())
        for a, b in (("requests", "batched"), ("requests_philox", "philox"), ("parent_batched", "batched"), ("parent_philox", "philox")):
            if a in outs:
                assert all(torch.equal(u, v) for u, v in zip(outs[a], outs[b])), (label, a, b)
        times = {name: [] for name in runs}
        for _ in range(args.reps):
            for name, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(round(e0.elapsed_time(e1) * 1e3 / args.launches, 3))
        for name, us in times.items():
            print(json.dumps({"shape": label, "entry": name, "launches": args.launches, "us_per_launch": us,
                              "min": min(us), "max": max(us)}), flush=True)


if __name__ == "__main__":
    main()
