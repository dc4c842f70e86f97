"""Bodies of the weight-packing tests (bbdm_amd/packing.py), run by tests/test_packing_emu_cpu.py on the CPU-emulated kernels and
by tests/test_packing_gpu.py on the GPU: every packer and plane layout the planner can construct, refreshed through the one
protocol.  Every comparison is bit-exact on the raw bytes of ``packed`` and of ``ubound`` / ``gain``: the same launches on the same
input are deterministic.

Shapes: the smallest the pack entry points take that still pad -- a weight [12, 20, k, k] (Cout not a whole 128-column block) under
32 input channels (Cin padded to whole 16-channel chunks).  The 1x1 data gradient arrives with 16 channels (its padded Cout: the
plane layouts take whole 16-channel chunks, 12 -> 16).  [8, 16, 3, 3] under 16 channels: the single-launch G g G^T -> planes kernels
at their smallest chunk count."""
import pytest
import torch
import torch.nn as nn

from bbdm_amd import _lib, packing

LAYOUTS = (False, True, "p", "h")
_LNAME = {False: "f32", True: "bf3", "p": "bf3p", "h": "h2p"}


def _specs():
    out = []
    for lay in LAYOUTS:
        out.append((f"conv1x1-{_LNAME[lay]}", "conv", (12, 20, 1, 1), dict(pad=32, layout=lay)))
        out.append((f"dgrad1x1-{_LNAME[lay]}", "conv", (12, 20, 1, 1), dict(pad=16, layout=lay, dgrad=True)))
    out.append(("conv3x3-f32", "conv", (12, 20, 3, 3), dict(pad=32)))               # the direct kernel's packing, both directions
    out.append(("dgrad3x3-f32", "conv", (12, 20, 3, 3), dict(pad=12, dgrad=True)))
    out.append(("linear-f32", "conv", (12, 20, 1), dict(pad=20)))                   # Conv1d weight [O, I, 1]
    for m in (2, 4, 6, 8):
        for lay in LAYOUTS:
            for dg in (False, True):
                out.append((f"wino{m}-{_LNAME[lay]}-{'dgrad' if dg else 'fwd'}", "wino", (12, 20, 3, 3),
                            dict(in_pad=32, m=m, bf3=lay, dgrad=dg)))
        for dg in (False, True):
            out.append((f"wino{m}-bf3p-{'dgrad' if dg else 'fwd'}-8x16", "wino", (8, 16, 3, 3), dict(in_pad=16, m=m, bf3="p", dgrad=dg)))
    # phase filters: every layout at m = 4 / 6; F(7x7, 2x2) exists on the pre-split planes only (_Plan._emit_conv)
    for m, lays in ((4, LAYOUTS), (6, LAYOUTS), (7, ("p", "h"))):
        for lay in lays:
            out.append((f"phases{m}-{_LNAME[lay]}", "wino", (12, 20, 3, 3), dict(in_pad=32, m=m, bf3=lay, phases=True)))
    out.append(("rowl1-bias", "rowl1", (12, 20, 1), dict(bias=True)))
    out.append(("rowl1-nobias", "rowl1", (12, 20, 1), dict(bias=False)))
    return out


SPECS = _specs()
params = pytest.mark.parametrize("spec", SPECS, ids=[s[0] for s in SPECS])


def _tensors(spec, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(*spec[2], generator=g) * 0.3).to(dev)
    b = torch.randn(spec[2][0], generator=g).to(dev)
    return w, b


def make(spec, weight: nn.Parameter, bias):
    _, kind, _, kw = spec
    if kind == "conv":
        return packing._PackedConv(weight, bias, **kw)
    if kind == "wino":
        return packing._PackedWinograd(weight, bias, **kw)
    return packing._RowL1Gain(weight, bias if kw["bias"] else None)


def build(spec, dev, seed=0):
    w, b = _tensors(spec, dev, seed)
    w, b = nn.Parameter(w), nn.Parameter(b)
    return make(spec, w, b), w, b


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def buffers(p, dev):
    """The raw bytes of everything a kernel reads from this packer."""
    _sync(dev)
    out = []
    for name in ("packed", "ubound", "gain"):
        t = getattr(p, name, None)
        if t is not None:
            out.append((name, t.detach().reshape(-1).view(torch.uint8).cpu().clone()))
    assert out
    return out


def same(a, b):
    assert [n for n, _ in a] == [n for n, _ in b]
    for (n, x), (_, y) in zip(a, b):
        assert torch.equal(x, y), n


def fresh(spec, p, dev):
    """Buffers of a newly constructed packer on the parameters ``p`` holds now."""
    q = make(spec, p.weight, p.bias)
    q.refresh(_lib.current_stream(dev))
    return buffers(q, dev)


def smaller_weights(dev, spec):
    """In-place update (the version moves, every bound shrinks): the refreshed buffers are those of a new packer.  Fails if ``ubound``
    is not zeroed before the maximum is accumulated into it."""
    p, w, b = build(spec, dev)
    stream = _lib.current_stream(dev)
    p.refresh(stream)
    before = buffers(p, dev)
    with torch.no_grad():
        w.mul_(0.5)
        b.mul_(0.5)
    p.refresh(stream)
    after = buffers(p, dev)
    same(after, fresh(spec, p, dev))
    assert any(not torch.equal(x, y) for (_, x), (_, y) in zip(before, after))        # (the update did reach the buffers)


def moved_storage(dev, spec):
    """``param.data`` swapped for another tensor, as EMA does: the storage changes, the version need not."""
    p, w, b = build(spec, dev)
    stream = _lib.current_stream(dev)
    p.refresh(stream)
    before = buffers(p, dev)
    w2, b2 = _tensors(spec, dev, seed=1)
    w.data, b.data = w2 * 0.5, b2 * 0.5
    p.refresh(stream)
    after = buffers(p, dev)
    same(after, fresh(spec, p, dev))
    assert any(not torch.equal(x, y) for (_, x), (_, y) in zip(before, after))


def no_change_no_launch(dev, spec):
    """A refresh with nothing changed issues no library call."""
    p, w, b = build(spec, dev)
    stream = _lib.current_stream(dev)
    calls = []
    orig = _lib.call

    def counting(name, *a):
        calls.append(name)
        return orig(name, *a)

    _lib.call = counting
    try:
        p.refresh(stream)
        first = len(calls)
        before = buffers(p, dev)
        p.refresh(stream)
        assert first > 0 and len(calls) == first, calls
    finally:
        _lib.call = orig
    same(buffers(p, dev), before)


def rejected_tensors(dev, spec):
    """Every packer refuses a weight (and a bias it reads) that is not contiguous fp32: the pack kernels take raw pointers."""
    w, b = _tensors(spec, dev)
    wide = torch.cat([w, w], 1)
    for bad in (wide[:, ::2], w.double()):
        assert bad.shape == w.shape and (not bad.is_contiguous() or bad.dtype != torch.float32)
        p = make(spec, nn.Parameter(bad), nn.Parameter(b))
        with pytest.raises(RuntimeError):
            p.refresh(_lib.current_stream(dev))
    if spec[1] == "rowl1" and spec[3]["bias"]:
        for bad in (torch.cat([b, b])[::2], b.double()):
            p = make(spec, nn.Parameter(w), nn.Parameter(bad))
            with pytest.raises(RuntimeError):
                p.refresh(_lib.current_stream(dev))


def second_stream(dev, spec):
    """GPU only.  Packed, then re-packed after an in-place update, on a second stream while torch's current stream is the default one
    (what the training plan does with its data-gradient operands): the same bytes as a packer refreshed on the current stream.  Every
    torch op of the packers (zeroing the bound, the transient scratch of the fp16-pair phase filters) must follow that stream."""
    p, w, b = build(spec, dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    p.refresh(side.cuda_stream)
    with torch.no_grad():
        side.synchronize()
        w.mul_(0.5)
        b.mul_(0.5)
    side.wait_stream(torch.cuda.current_stream(dev))
    p.refresh(side.cuda_stream)
    side.synchronize()
    same(buffers(p, dev), fresh(spec, p, dev))
