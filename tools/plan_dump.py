"""Canonical text form of a matrix of execution plans (UNet inference / training, the tiny golden models, the first stage), built on
CPU tensors against the emulated library: run it on two commits and compare the outputs byte by byte -- a planner refactor must not
move one launch or one argument.  Prints the dump; its line count and sha256 go to stderr.  `plan_dump.py c3` = titles containing c3."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import bench                                                                            # noqa: E402
from bbdm_amd import unet as U                                                          # noqa: E402
from emu_backend import emulated_backend                                                # noqa: E402

CPU = torch.device("cpu")
FLIPS = ([(k, 0) for k in ("gemm_h2", "gemm_bf3p", "gemm_bf3", "winograd_wgrad")] + [("gemm_h2_train", v) for v in range(4)] +
         [(k, 0) for k in ("side_stream_train", "side_stream_wgrad", "upsample_phases", "upsample_f72", "gn_in_transform", "conv1x1_small",
                           "conv1x1_h2", "winograd_fuse_groupnorm", "fuse_stats")])
SIZES = ("_wino_v", "_wino_m", "_conv_ws", "_conv_ws_floats", "_h2_bounds", "_ws_f", "_ws_f_floats", "_ws_f_side", "_ws_f_side_floats",
         "_ws_d", "_ws_d2")


def dump(title, plan, params):
    """One plan as lines of text: objects are numbered in their order of first appearance, parameters by their place in ``params``."""
    seen, pidx = {"b": {}, "t": {}}, {id(p): k for k, p in enumerate(params)}

    def num(kind, o):
        return seen[kind].setdefault(id(o), len(seen[kind]))

    def r(a):
        if isinstance(a, U._View):
            return f"V({num('b', a.buf)},{a.off},{a.ld},{a.N},{a.H},{a.W},{a.C})"
        if isinstance(a, U._TensorRef):
            t = a.t.t if isinstance(a.t, U._LateTensor) else a.t
            return f"T({num('t', a.t)},{a.byte_off},{t.numel()})"
        if isinstance(a, U._ParamRef):
            return f"P({pidx.get(id(a.p))},{tuple(a.p.shape)})"
        if isinstance(a, U._LateTensor):
            return f"L({num('t', a)},{a.t.numel()})"
        if isinstance(a, U._LateInt):
            return f"I({a.v})"
        if isinstance(a, (U._Plan._StatsRef, U._Plan._H2Ref, U._Plan._GradRef)):
            return type(a).__name__ + str(tuple(getattr(a, s) for s in a.__slots__ if s != "plan"))
        return repr(a)

    out = [f"== {title}"]
    for tag in ("ops", "bops", "bops_x0"):
        out += [f"{tag} {n} {getattr(n, 'entry', '')} " + " ".join(map(r, a)) for n, a in getattr(plan, tag, [])]
    out.append(f"side {plan._side_ranges} bside {getattr(plan, '_bside_ranges', None)} bsegs {[s[:2] for s in getattr(plan, 'bsegs', [])]}")
    out.append(f"bufs {[b.numel for b in plan.bufs]}")
    out.append("sizes " + " ".join(f"{k}={r(getattr(plan, k))}" for k in SIZES if hasattr(plan, k)))
    out.append(f"gn {plan._gn_count} h2 {len(plan._h2_layers)} x {plan._h2_x_slots} dy {plan._h2_dy_slots} "
               f"fused_train {sorted(pidx[i] for i in plan._fused_train)}")
    for k, p in enumerate(params):
        v = plan._saved_V.get(id(p))
        if v is not None:
            out.append(f"savedV {k} {r(v[0])} m={v[1]} transposed={len(v) > 2 and bool(v[2])} bound={r(v[3]) if len(v) > 3 else None}")
    for tag in ("convs", "dconvs"):
        out += [f"{tag} {type(c).__name__} w={pidx.get(id(c.weight))} bf3={getattr(c, 'bf3', None)} "
                f"planes={getattr(getattr(c, 'planes', None), 'entry', None)} m={getattr(c, 'm', None)} phases={getattr(c, 'phases', None)} "
                f"dgrad={getattr(c, 'dgrad', None)} pad={getattr(c, 'in_pad', getattr(c, 'pad', None))}" for c in getattr(plan, tag, [])]
    return out


def matrix():
    for w, (_, up, ch, size, n, *_) in sorted(bench.WORKLOADS.items()):
        m = U.UNetModel(**up)
        m.max_cached_plans = 1
        cases = [("winograd", c, b) for b in (n, 2) for c in (0, 4, 6, 8)] + [(k, v, n) for k, v in FLIPS if w in ("c1", "c3")]
        for k, v, b in cases:
            old = getattr(m, k)
            setattr(m, k, v)
            for training in (False, True):
                yield f"{w} batch {b} {'train' if training else 'infer'} {k}={v}", m._plan_for(torch.zeros(b, ch, size, size), training), m
            setattr(m, k, old)
    import test_training_gpu as T
    from fixtures import load_case
    for name in ("tiny_concat", "tiny_nocond", "tiny_xattn", "tiny_ysubx"):
        rec = load_case(name)
        fn = T.build(rec, CPU).denoise_fn
        for band in (0, 1 << 62):                        # (the second pass: every skip projection inside the side-stream band)
            fn.side_stream_min_macs, fn.side_stream_max_macs, fn.side_stream_max_pixels = 0, band, band
            for training in (False, True):
                yield f"{name} {'train' if training else 'infer'} band={band}", fn._plan_for(rec["x0"], training), fn
    import first_stage_cases as C
    vq = C.make(CPU, resolution=16, attn_resolutions=[8])
    for kind, shape in (("encode", (1, 3, 32, 32)), ("decode", (1, 4, 8, 8))):
        for qc in (True, False):
            yield f"first stage {kind} quant_conv={qc}", vq._plan(kind, torch.zeros(shape), qc), vq


if __name__ == "__main__":
    sha, lines = hashlib.sha256(), 0
    with emulated_backend():
        for title, plan, model in matrix():
            if all(s in title for s in sys.argv[1:]):
                text = "\n".join(dump(title, plan, list(model.parameters()))) + "\n"
                sys.stdout.write(text)
                sha.update(text.encode())
                lines += text.count("\n")
    print(f"plan_dump: {lines} lines, sha256 {sha.hexdigest()}", file=sys.stderr)
