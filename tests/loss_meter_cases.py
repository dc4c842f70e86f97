"""Shared bodies of the loss-meter tests (csrc/loss_meter.hip, bbdm_amd/loss_meter.py, the hook in BrownianBridgeModel._denoise_and_loss):
run on the CPU-emulated kernels by tests/test_loss_meter_emu_cpu.py and on the GPU by tests/test_loss_meter_gpu.py -- TEST
INFRASTRUCTURE.

Kernel-level shapes (per_sample; a workgroup sums one 2048-element chunk of one image, LM_CHUNK in csrc/loss_meter.hip):
  192  = 3 x 8 x 8    16-byte loads, one block per image
  75   = 3 x 5 x 5    element loads, a last group of three elements
  3072 = 3 x 32 x 32  two blocks per image (the first size of the table above 2048), the second one half filled
  192 with ``a`` a view one float past an allocation: a vector-sized per_sample on a misaligned pointer -> element loads
each with N = 1 and N = 5, both loss types, inputs randn under a fixed seed.

Bounds.  The kernel forms a - b in fp32 and sums |d| or d^2 in fp64, so the fp64 references are formed from ``(a - b).double()``.
The kernel's summation order differs from torch's: at most per_sample * 2^-53 relative (non-negative terms).  Per-image fp32 value:
that is far below fp32's half ulp, so the result is within one fp32 ulp of the reference, relative 2^-23.  Bucket sums:
per_sample * 2^-52 (the same bound doubled for the division by per_sample), sums of squares twice that.  Everything else is bitwise."""
import functools
import math

import pytest
import torch

from fixtures import load_case
from philox_cases import _offset

KERNEL_SHAPES = [(192, 0), (75, 0), (3072, 0), (192, 1)]            # (per_sample, offset of `a` in floats)
KERNEL_IDS = ["192-vec", "75-elem", "3072-two-blocks", "192-misaligned"]
TABLES = [(1000, 10), (1000, 7), (10, 4)]                           # (T, B)
LOSS_TYPES = ["l1", "l2"]


@functools.lru_cache(maxsize=None)
def pair(n, per_sample, seed=0):
    """(a, b) fp32 [n, per_sample] on the CPU (computed once per case and shared; never modified)."""
    g = torch.Generator().manual_seed(1000 * per_sample + 10 * n + seed)
    return torch.randn(n, per_sample, generator=g), torch.randn(n, per_sample, generator=g)


def image_refs(a, b, loss_type):
    """float64 [N]: the per-image mean of |a - b| or (a - b)^2 with the difference formed in fp32, as the kernel forms it."""
    d = (a - b).double()
    return (d.abs() if loss_type == "l1" else d * d).mean(1)


def on_device(a, b, dev, off=0):
    a, b = a.to(dev), b.to(dev)
    if off:
        a = _offset(a, off)
        assert a.data_ptr() % 16 != 0 and a.is_contiguous()
    return a, b


# ---- case 1 ------------------------------------------------------------------------------------------------------------------
def per_image_values(dev, per_sample, off, n, loss_type):
    from bbdm_amd import per_image_loss
    a, b = pair(n, per_sample)
    ref = image_refs(a, b, loss_type)
    got = per_image_loss(*on_device(a, b, dev, off), loss_type)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
    rel = ((got.double().cpu() - ref).abs() / ref)
    print(f"per_image {per_sample} off {off} N {n} {loss_type}: max rel err {float(rel.max()):.3e} (bar {2.0 ** -23:.3e})")
    assert bool((rel <= 2.0 ** -23).all()), rel.tolist()


# ---- case 2 ------------------------------------------------------------------------------------------------------------------
def edge_timesteps(T, B):
    """0, T - 1 and every bucket edge with its two neighbours, in range."""
    ts = {0, T - 1}
    for bucket in range(1, B):
        e = -((-bucket * T) // B)                                  # the smallest t with (t * B) // T >= bucket
        ts.update(v for v in (e - 1, e, e + 1) if 0 <= v < T)
    return sorted(ts)


def bucket_table(dev, T, B, loss_type, per_sample=75):
    from bbdm_amd import LossMeter
    ts = edge_timesteps(T, B)
    n = len(ts)
    a, b = pair(n, per_sample, seed=T + B)
    ref = image_refs(a, b, loss_type).tolist()
    meter = LossMeter(T, B, device=dev, loss_type=loss_type)
    assert meter.add(*on_device(a, b, dev), torch.tensor(ts, dtype=torch.int64, device=dev)) is None
    sums, counts = meter._read_sums()
    want_count = [0] * B
    per_bucket = [[] for _ in range(B)]
    for v, t in zip(ref, ts):
        want_count[(t * B) // T] += 1
        per_bucket[(t * B) // T].append(v)
    assert counts.tolist() == want_count + [0]
    tol = per_sample * 2.0 ** -52
    for k in range(B):
        s_ref, q_ref = math.fsum(per_bucket[k]), math.fsum(v * v for v in per_bucket[k])
        s, q = float(sums[0, k]), float(sums[1, k])
        print(f"T {T} B {B} bucket {k}: n {want_count[k]} sum rel err {abs(s - s_ref) / max(s_ref, 1e-300):.3e} (bar {tol:.3e}) "
              f"sumsq rel err {abs(q - q_ref) / max(q_ref, 1e-300):.3e}")
        assert abs(s - s_ref) <= tol * s_ref and abs(q - q_ref) <= 2 * tol * q_ref, (k, s, s_ref, q, q_ref)
    r = meter.read()
    assert r["count"].tolist() == want_count and r["rejected"] == 0 and r["count"].dtype == torch.int64
    assert r["edges"].tolist() == [min(t for t in range(T) if (t * B) // T >= k) if any((t * B) // T >= k for t in range(T)) else T
                                   for k in range(B)] + [T]
    for k in range(B):
        if want_count[k] == 0:
            assert math.isnan(float(r["mean"][k])) and math.isnan(float(r["stderr"][k]))
            continue
        m = float(sums[0, k]) / want_count[k]
        assert float(r["mean"][k]) == m
        assert float(r["stderr"][k]) == math.sqrt(max(float(sums[1, k]) / want_count[k] - m * m, 0.0) / want_count[k])
    assert r["mean"].dtype == torch.float64 and r["stderr"].dtype == torch.float64
    assert abs(r["loss"] - math.fsum(ref) / n) <= tol * r["loss"]


# ---- case 3 ------------------------------------------------------------------------------------------------------------------
def order_and_batching(dev, per_sample, loss_type):
    """15 (a, b, t) triples as one batch, permuted, in pieces of 1, 3, 5, 6 images and from a misaligned copy of ``a`` (element loads
    of the same groups): the int64 state is the same, bit for bit."""
    from bbdm_amd import LossMeter
    T, B = 1000, 10
    a, b = on_device(*pair(15, per_sample), dev)
    t = torch.tensor([0, 999, 99, 100, 101, 500, 499, 37, 37, 640, 905, 250, 251, 777, 12], dtype=torch.int64, device=dev)
    new = lambda: LossMeter(T, B, device=dev, loss_type=loss_type)
    whole = new()
    whole.add(a, b, t)
    perm = torch.randperm(15, generator=torch.Generator().manual_seed(3)).to(dev)
    assert not torch.equal(perm.cpu(), torch.arange(15))
    permuted = new()
    permuted.add(a[perm].contiguous(), b[perm].contiguous(), t[perm])
    pieces, at = new(), 0
    for size in (1, 3, 5, 6):
        pieces.add(a[at:at + size], b[at:at + size], t[at:at + size])
        at += size
    assert at == 15
    shifted = new()
    shifted.add(_offset(a, 1), b, t)
    assert int(whole.counts.sum()) == 15 and bool((whole.meter[:, 0, :3] != 0).any())
    for other, name in ((permuted, "permuted"), (pieces, "pieces"), (shifted, "misaligned")):
        assert torch.equal(other.meter, whole.meter) and torch.equal(other.counts, whole.counts), name
        assert other.meter.dtype == torch.int64 and tuple(other.meter.shape) == (B, 2, 4) and tuple(other.counts.shape) == (B + 1,)


# ---- case 4 ------------------------------------------------------------------------------------------------------------------
def rejected_timesteps(dev):
    """t in {-1, T, T + 5, 2^40 + 3} next to valid values: the buckets equal those of the valid images alone, rejected == 4.  With
    T = 1000 the last value would land in bucket 0 if it were narrowed to 32 bits before the comparison."""
    from bbdm_amd import LossMeter
    T, B = 1000, 10
    a, b = on_device(*pair(9, 192), dev)
    t = torch.tensor([5, -1, 999, T, 420, T + 5, 2 ** 40 + 3, 421, 0], dtype=torch.int64, device=dev)
    valid = torch.tensor([0, 2, 4, 7, 8], device=dev)
    mixed, alone = LossMeter(T, B, device=dev), LossMeter(T, B, device=dev)
    mixed.add(a, b, t)
    alone.add(a[valid].contiguous(), b[valid].contiguous(), t[valid])
    assert torch.equal(mixed.meter, alone.meter) and torch.equal(mixed.counts[:B], alone.counts[:B])
    r = mixed.read()
    assert r["rejected"] == 4 and int(r["count"].sum()) == 5 and alone.read()["rejected"] == 0
    assert r["count"].tolist() == [2, 0, 0, 0, 2, 0, 0, 0, 0, 1]


# ---- case 5 ------------------------------------------------------------------------------------------------------------------
def non_finite(dev):
    from bbdm_amd import LossMeter
    T, B = 1000, 10
    a, b = pair(6, 192)
    t = torch.tensor([10, 150, 151, 480, 950, 951], dtype=torch.int64, device=dev)
    bad = a.clone()
    bad[2, 77] = float("inf")                                  # image 2: bucket 1, next to the finite image 1
    clean, meter = LossMeter(T, B, device=dev), LossMeter(T, B, device=dev)
    keep = [0, 3, 4, 5]
    clean.add(a[keep].to(dev), b[keep].to(dev), t[keep])
    meter.add(bad.to(dev), b.to(dev), t)
    r, c = meter.read(), clean.read()
    assert math.isnan(float(r["mean"][1])) and math.isnan(float(r["stderr"][1])) and math.isnan(r["loss"])
    assert r["count"].tolist() == [1, 2, 0, 0, 1, 0, 0, 0, 0, 2]
    others = [k for k in range(B) if k != 1]
    assert torch.equal(meter.meter[others], clean.meter[others])
    for k in (0, 4, 9):
        assert float(r["mean"][k]) == float(c["mean"][k]) and float(r["stderr"][k]) == float(c["stderr"][k])
    meter.reset()
    assert not bool(meter.meter.any()) and not bool(meter.counts.any())
    meter.add(a.to(dev), b.to(dev), t)
    r = meter.read()
    assert bool(torch.isfinite(r["mean"][[0, 1, 4, 9]]).all()) and math.isfinite(r["loss"]) and float(r["mean"][1]) > 0


# ---- case 6 ------------------------------------------------------------------------------------------------------------------
def merge_and_state_dict(dev):
    from bbdm_amd import LossMeter
    T, B = 1000, 7
    a, b = on_device(*pair(10, 75), dev)
    t = torch.tensor([0, 999, 142, 143, 500, 501, 857, 858, 3, 3], dtype=torch.int64, device=dev)
    whole, lo, hi = (LossMeter(T, B, device=dev, loss_type="l2") for _ in range(3))
    whole.add(a, b, t)
    lo.add(a[:5], b[:5], t[:5])
    hi.add(a[5:], b[5:], t[5:])
    assert not torch.equal(lo.meter, whole.meter)
    assert lo.merge(hi) is lo
    assert torch.equal(lo.meter, whole.meter) and torch.equal(lo.counts, whole.counts)
    state = whole.state_dict()
    assert state["num_timesteps"] == T and state["buckets"] == B
    assert state["meter"].dtype == torch.int64 and state["counts"].dtype == torch.int64
    back = LossMeter(T, B, device=dev, loss_type="l2")
    back.load_state_dict(state)
    assert torch.equal(back.meter, whole.meter) and torch.equal(back.counts, whole.counts) and back.meter.device == whole.meter.device
    r1, r2 = back.read(), whole.read()
    assert torch.equal(r1["count"], r2["count"]) and r1["loss"] == r2["loss"]
    assert torch.equal(r1["mean"].nan_to_num(-1.0), r2["mean"].nan_to_num(-1.0))
    whole.meter[0, 0, 0] += 1                                    # the state dict holds copies
    assert not torch.equal(state["meter"], whole.meter.cpu())
    for other in (LossMeter(T, B + 1, device=dev), LossMeter(T + 1, B, device=dev)):
        with pytest.raises(ValueError):
            other.load_state_dict(state)
        with pytest.raises(ValueError):
            other.merge(back)
    full = LossMeter(T, B, device=dev)
    full.counts[2] = 1 << 23
    with pytest.raises(OverflowError):
        full.read()
    full.counts[2] -= 1
    full.read()


# ---- case 7 ------------------------------------------------------------------------------------------------------------------
def _ns(c):
    import argparse
    ns = argparse.Namespace()
    for k, v in c.items():
        setattr(ns, k, _ns(v) if isinstance(v, dict) else v)
    return ns


@functools.lru_cache(maxsize=None)
def pixel_model(dev):
    """A pixel BBDM in the style of the golden tiny_concat case of tests/sampler_cases.py (its bridge parameters, condition_key
    SpatialRescaler: context = y, concatenated), with a one-level UNet on 8 x 8 images and synthetic weights: the emulator spends
    seconds per UNet call whatever the batch, and nothing the meter does depends on the UNet's depth -> (model, x0 [3], y [3])."""
    import bbdm_amd
    from fixture_weights import synth_weights
    rec = load_case("tiny_concat")
    up = dict(rec["unet_params"], image_size=8, model_channels=32, num_res_blocks=1, attention_resolutions=(), channel_mult=(1,),
              num_heads=2, num_head_channels=-1)
    assert up["condition_key"] != "nocond"
    m = bbdm_amd.BrownianBridgeModel(_ns({"BB": {"params": dict(rec["bb_params"], UNetParams=up)}}))
    m.denoise_fn.load_state_dict(synth_weights([(k, tuple(v.shape)) for k, v in m.denoise_fn.state_dict().items()], 44), strict=True)
    m = m.to(dev).eval()
    if dev.type == "cpu":
        m.denoise_fn.hip_graph = False                          # hipGraph capture needs a real device
    g = torch.Generator().manual_seed(62)
    x0, y = (torch.randn(3, 3, 8, 8, generator=g).clamp(-1, 1) for _ in range(2))
    return m, x0, y


def _train_step(m, fn, seed):
    for p in m.denoise_fn.parameters():
        p.grad = None
    torch.manual_seed(seed)
    loss, log = fn()
    loss.backward()
    grads = {k: p.grad.clone() for k, p in m.denoise_fn.named_parameters()}
    for p in m.denoise_fn.parameters():
        p.grad = None
    assert len(grads) > 0 and any(float(g.abs().max()) > 0 for g in grads.values())
    return loss.detach().clone(), grads, sorted(log)


def _attach_changes_nothing(m, dev, step, eval_call, batch):
    from bbdm_amd import LossMeter
    train, val = LossMeter(m.num_timesteps, 10, device=dev), LossMeter(m.num_timesteps, 10, device=dev)
    m.train()
    try:
        loss0, grads0, keys0 = _train_step(m, step, 21)
        m.attach_loss_meter(train=train, val=val)
        loss1, grads1, keys1 = _train_step(m, step, 21)
        assert bool(torch.isfinite(loss0)) and torch.equal(loss1, loss0) and keys1 == keys0 == ["loss", "x0_recon"]
        for k, g in grads0.items():
            assert torch.equal(grads1[k], g), k
        r = train.read()
        scalar = float(loss0.double())
        print(f"scalar loss {scalar!r}, meter loss {r['loss']!r}: rel {abs(r['loss'] - scalar) / scalar:.3e} (bar {2.0 ** -23:.3e})")
        assert int(r["count"].sum()) == batch and r["rejected"] == 0 and not bool(val.counts.any())
        assert abs(r["loss"] - scalar) <= 2.0 ** -23 * scalar
        m.eval()
        with torch.no_grad():
            torch.manual_seed(22)
            eval_call()
        assert int(val.read()["count"].sum()) == batch and int(train.read()["count"].sum()) == batch
        m.detach_loss_meter()
        assert m._loss_meters == (None, None)
        with pytest.raises(ValueError):
            m.attach_loss_meter(train=LossMeter(m.num_timesteps + 1, 10, device=dev))
    finally:
        m.detach_loss_meter()
        m.eval()


def attach_changes_nothing_pixel(dev):
    m, x0, y = pixel_model(dev)
    x0, y = x0.to(dev), y.to(dev)
    _attach_changes_nothing(m, dev, lambda: m(x0, y), lambda: m(x0, y), x0.shape[0])


def attach_changes_nothing_latent(dev):
    import latent_cache_cases as L
    m, ds, cache = L.shared(dev)
    x, c = ds.x[4:8].to(dev), ds.c[4:8].to(dev)
    try:
        _attach_changes_nothing(m, dev, lambda: m(x, c), lambda: m(x, c), 4)
    finally:
        m.train()                                               # the shared latent model is kept in training mode


def out_of_range_t_reads_no_memory_beside_the_tables(dev):
    """q_sample (tensor noise and seeds) and predict_x0_from_objective with t outside [0, T) equal the same calls with t clamped, bit
    for bit: the kernels index the schedule tables with the clamped value, not with whatever lies beside them."""
    m, x0, y = pixel_model(dev)
    T = m.num_timesteps
    x0, y = x0.to(dev), y.to(dev)
    noise = torch.randn(x0.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    bad = torch.tensor([-1, T + 949, 2 ** 40 + 3], dtype=torch.int64, device=dev)
    good = torch.tensor([0, T - 1, T - 1], dtype=torch.int64, device=dev)
    for kw in ({"noise": noise}, {"seeds": [5, 6, 7], "ordinals": 2}):
        got, want = m.q_sample(x0, y, bad, **kw), m.q_sample(x0, y, good, **kw)
        assert bool(torch.isfinite(want[0]).all()) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(m.predict_x0_from_objective(x0, y, bad, noise), m.predict_x0_from_objective(x0, y, good, noise))


# ---- case 8 ------------------------------------------------------------------------------------------------------------------
VAL_IDX = [0, 1, 2, 5, 2 ** 31 + 1, 2 ** 31 + 2]


def timestep_formula(T, idx, t_offset):
    return ((((idx + t_offset) * 2654435761) & 0xFFFFFFFF) * T) >> 32


def validation_timesteps_match_the_formula():
    from bbdm_amd.loss_meter import validation_timesteps
    for T in (1000, 10, 1):
        for off in (0, 7, 2 ** 31):
            idx = VAL_IDX + [2 ** 32 - 1, 2 ** 33 + 12345, 999]
            got = validation_timesteps(torch.tensor(idx, dtype=torch.int64), T, off)
            assert got.dtype == torch.int64 and got.tolist() == [timestep_formula(T, i, off) for i in idx]
            assert all(0 <= v < T for v in got.tolist())
    spread = validation_timesteps(torch.arange(1000), 1000).tolist()
    assert len(set(v // 100 for v in spread[:10])) >= 6         # consecutive indices do not share a bucket


def validation_loss_pixel(dev):
    """Two runs over the same 6 items: equal states; the t it used is the formula in Python integers; the state equals that of a loop
    written out here -- p_losses under eval() and no_grad with that t, seeds = base_seed + idx and ordinal 0, feeding a meter through
    the hook -- and, for the first batch, q_sample, the UNet and meter.add called by hand."""
    from bbdm_amd import LossMeter, validation_loss
    m, x0, y0 = pixel_model(dev)
    T, base_seed, t_offset = m.num_timesteps, 1234, 3
    xs, ys = torch.cat([x0, y0.flip(0)]), torch.cat([y0, x0.flip(0)])
    idx = torch.tensor(VAL_IDX, dtype=torch.int64)
    batches = [(xs[s], ys[s], idx[s]) for s in (slice(0, 2), slice(2, 6))]
    m.train()
    try:
        runs = [validation_loss(m, batches, LossMeter(T, 10, device=dev), base_seed, t_offset) for _ in range(2)]
        assert m.training and m._loss_meters == (None, None)
    finally:
        m.eval()
    assert torch.equal(runs[0].meter, runs[1].meter) and torch.equal(runs[0].counts, runs[1].counts)
    assert int(runs[0].counts.sum()) == 6 and int(runs[0].counts[10]) == 0
    want_count = [0] * 10
    for i in VAL_IDX:
        want_count[timestep_formula(T, i, t_offset) * 10 // T] += 1
    assert runs[0].read()["count"].tolist() == want_count
    hooked, by_hand, first = LossMeter(T, 10, device=dev), LossMeter(T, 10, device=dev), None
    with torch.no_grad():
        for x, y, ix in batches:
            x, y = x.to(dev), y.to(dev)
            ctx = None if m.condition_key == "nocond" else y     # the context forward() forms
            t = torch.tensor([timestep_formula(T, i, t_offset) for i in ix.tolist()], dtype=torch.int64, device=dev)
            seeds = [base_seed + i for i in ix.tolist()]
            m.attach_loss_meter(val=hooked)
            try:
                m.p_losses(x, y, ctx, t, seeds=seeds, ordinals=0)
            finally:
                m.detach_loss_meter()
            if first is None:
                first = (hooked.meter.clone(), hooked.counts.clone())
                x_t, objective = m.q_sample(x, y, t, seeds=seeds, ordinals=0)
                by_hand.add(objective, m.denoise_fn(x_t, timesteps=t, context=ctx), t, loss_type=m.loss_type)
    assert torch.equal(by_hand.meter, first[0]) and torch.equal(by_hand.counts, first[1]) and int(first[1].sum()) == 2
    assert torch.equal(hooked.meter, runs[0].meter) and torch.equal(hooked.counts, runs[0].counts)


def validation_loss_latent_cache(dev):
    """The latent model fed cache rows gives the state of the same model fed the images the rows were encoded from (batches of four
    consecutive items, as the cache was built)."""
    import latent_cache_cases as L
    from bbdm_amd import LossMeter, validation_loss
    m, ds, cache = L.shared(dev)
    T = m.num_timesteps
    spans = [(0, 4), (4, 8)]
    images = [(ds.x[b:e], ds.c[b:e], torch.arange(b, e)) for b, e in spans]
    rows = [(torch.arange(b, e, device=dev), torch.arange(b, e, device=dev), torch.arange(b, e)) for b, e in spans]
    try:
        from_images = validation_loss(m, images, LossMeter(T, 10, device=dev), base_seed=77)
        m.attach_latent_cache(cache)
        from_rows = validation_loss(m, rows, LossMeter(T, 10, device=dev), base_seed=77)
        assert m.training
    finally:
        m.detach_latent_cache()
        m.train()
    assert int(from_images.counts.sum()) == 8 and bool(torch.isfinite(from_images.read()["mean"].nan_to_num(0.0)).all())
    assert torch.equal(from_rows.meter, from_images.meter) and torch.equal(from_rows.counts, from_images.counts)
