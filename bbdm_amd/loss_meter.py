"""The loss by timestep, accumulated on the device (``csrc/loss_meter.hip``).

The reference logs one scalar per micro-step -- the batch mean of the loss at whatever ``t`` each image drew
(BrownianBridgeModel.py:114-117) -- and reads it back every step for the progress bar and ``scheduler.step``
(BaseRunner.py:417-436).  Its validation loss (``validation_epoch``, BaseRunner.py:214-249) calls ``net(x, x_cond)``, which draws
fresh ``t`` and fresh noise: two evaluations of one checkpoint differ.

* :class:`LossMeter`        -- a table over ``buckets`` ranges of ``t``: count, sum and sum of squares of the per-image loss, kept on
  the device as exact integer limbs.  ``add`` enqueues two small launches and never reads back; ``read`` is the one call that syncs.
  The table is a function of the multiset of (image loss, t) it was fed: the same bits for any batch size, arrival order or split
  over ranks (``merge`` / ``all_reduce`` add the integers).
* :func:`per_image_loss`    -- the per-image mean of ``|a - b|`` / ``(a - b)^2`` alone.
* :func:`validation_loss`   -- a validation pass whose ``t`` and noise are functions of the dataset index:
  the result depends on the checkpoint, the dataset and two integers.

``BrownianBridgeModel.attach_loss_meter(train=, val=)`` makes every loss evaluation of the model feed a meter; with none attached the
model does what it did before.  The scalar loss and its kernel are untouched either way.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional

import torch

from . import _lib

__all__ = ["LossMeter", "per_image_loss", "validation_loss", "validation_timesteps"]

_SA_W = 4                    # 64-bit words of one accumulator cell (csrc/stats_acc.h)
_LOSSES = {"l1": 0, "l2": 1}
MAX_COUNT = 1 << 23          # additions a limb cell takes before a limb could wrap (csrc/stats_acc.h)
_HASH = 2654435761           # Knuth's multiplicative constant, floor(2^32 / golden ratio)


def _launch(t: torch.Tensor, name: str, *args):
    with _lib.device_guard(t.device):
        _lib.call(name, *args, _lib.current_stream(t.device))


def _f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def _as_int64(v: int) -> int:
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def _image_cells(a: torch.Tensor, b: torch.Tensor, loss_type, per_image: bool):
    """-> (cells int64 [N, 4], per-image fp32 [N] or None, per_sample) for two equal-shaped batches ``[N, ...]``."""
    if loss_type not in _LOSSES:
        raise NotImplementedError(f"loss_type {loss_type!r}: 'l1' or 'l2'")
    if a.shape != b.shape or a.dim() < 2:
        raise ValueError(f"expected two equal [N, ...] batches, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.device != b.device:
        raise ValueError("the two batches live on different devices")
    _lib.require_gpu(a, b)
    a, b = _f32c(a), _f32c(b)
    n = a.shape[0]
    per_sample = a[0].numel() if n else 0
    cells = torch.zeros(n, _SA_W, dtype=torch.int64, device=a.device)
    out = torch.empty(n, dtype=torch.float32, device=a.device) if per_image else None
    if n and per_sample:
        _launch(a, "bbdm_loss_meter_per_image_f32", a.data_ptr(), b.data_ptr(), cells.data_ptr(), None if out is None else out.data_ptr(),
                n, per_sample, _LOSSES[loss_type])
    return cells, out, per_sample


@torch.no_grad()
def per_image_loss(a: torch.Tensor, b: torch.Tensor, loss_type: str = "l1") -> torch.Tensor:
    """fp32 ``[N]``: the mean over each image of ``|a - b|`` (``'l1'``) or ``(a - b)^2`` (``'l2'``) -- the difference in fp32, the sum
    in fp64, rounded once.  A function of the image's values alone."""
    return _image_cells(a, b, loss_type, True)[1]


class LossMeter:
    """``LossMeter(num_timesteps, buckets=10, device=..., loss_type='l1')``: the per-image loss by bucket of ``t``.

    Bucket of ``t``: ``(t * buckets) // num_timesteps``.  ``add(a, b, t)`` adds the images of a batch (``a``, ``b``: ``[N, ...]`` fp32,
    ``t``: int64 ``[N]`` on the device) without a host read-back; a ``t`` outside ``[0, num_timesteps)`` touches no bucket and is
    counted in ``rejected``; a non-finite image loss makes its bucket read NaN until ``reset()``.  ``read()`` syncs and returns the
    table.  State: ``meter`` int64 ``[buckets, 2, 4]`` (sum and sum of squares as limb cells) and ``counts`` int64 ``[buckets + 1]``."""

    def __init__(self, num_timesteps: int, buckets: int = 10, device=None, loss_type: str = "l1"):
        T, B = int(num_timesteps), int(buckets)
        if T < 1 or B < 1 or T >= 1 << 31 or B >= 1 << 30:
            raise ValueError(f"num_timesteps={num_timesteps} and buckets={buckets} must be positive 32-bit integers")
        if loss_type not in _LOSSES:
            raise NotImplementedError(f"loss_type {loss_type!r}: 'l1' or 'l2'")
        self.num_timesteps, self.buckets, self.loss_type = T, B, loss_type
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.meter = torch.zeros(B, 2, _SA_W, dtype=torch.int64, device=device)
        self.counts = torch.zeros(B + 1, dtype=torch.int64, device=device)

    @property
    def device(self):
        return self.meter.device

    @torch.no_grad()
    def add(self, a: torch.Tensor, b: torch.Tensor, t: torch.Tensor, loss_type: Optional[str] = None, per_image: bool = False):
        """Two launches on the current stream, no sync.  ``per_image=True`` also returns the fp32 ``[N]`` image losses."""
        cells, out, per_sample = _image_cells(a, b, self.loss_type if loss_type is None else loss_type, per_image)
        n = cells.shape[0]
        if cells.device != self.meter.device:
            raise ValueError(f"the meter lives on {self.meter.device}, the batch on {cells.device}")
        if not isinstance(t, torch.Tensor) or torch.is_floating_point(t) or t.numel() != n:
            raise ValueError(f"t must be an integer tensor with one entry per image ({n})")
        tc = t.reshape(-1).to(device=cells.device, dtype=torch.int64).contiguous()
        if n and per_sample:
            _lib.require_gpu(tc, self.meter)
            _launch(cells, "bbdm_loss_meter_accumulate", cells.data_ptr(), tc.data_ptr(), self.meter.data_ptr(), self.counts.data_ptr(),
                    n, per_sample, self.num_timesteps, self.buckets)
        return out

    def edges(self) -> torch.Tensor:
        """int64 ``[buckets + 1]``: the smallest ``t`` of each bucket, then ``num_timesteps``."""
        T, B = self.num_timesteps, self.buckets
        return torch.tensor([-((-b * T) // B) for b in range(B)] + [T], dtype=torch.int64)

    def _read_sums(self):
        """-> (float64 [2, B] = the folded sums and sums of squares, int64 [B + 1] counts), on the host."""
        B = self.buckets
        sums = torch.empty(2, B, dtype=torch.float64, device=self.meter.device)
        _lib.require_gpu(self.meter)
        _launch(self.meter, "bbdm_loss_meter_read", self.meter.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), B)
        return sums.cpu(), self.counts.cpu()

    def read(self) -> Dict[str, object]:
        """The one call that syncs.  ``count`` int64 [B]; ``mean`` float64 [B] (NaN for an empty bucket); ``stderr`` float64 [B] =
        ``sqrt(max(sumsq / n - mean^2, 0) / n)``; ``edges`` int64 [B + 1]; ``loss`` = the sum of the sums / the sum of the counts;
        ``rejected``.  Raises ``OverflowError`` once 2^23 images were added since the last ``reset()``."""
        B = self.buckets
        sums, counts = self._read_sums()
        count, rejected = counts[:B].clone(), int(counts[B])
        total = int(count.sum())
        if total >= MAX_COUNT:
            raise OverflowError(f"{total} images since the last reset(): the limb cells guarantee {MAX_COUNT} additions")
        # Python floats: IEEE division and a correctly rounded square root, so equal states read as equal numbers on every host
        # (torch's vectorised CPU sqrt is not correctly rounded on every build)
        mean, stderr = [math.nan] * B, [math.nan] * B
        for k, (s, q, n) in enumerate(zip(sums[0].tolist(), sums[1].tolist(), count.tolist())):
            if n:
                mean[k] = s / n
                var = q / n - mean[k] * mean[k]
                stderr[k] = math.nan if math.isnan(var) else math.sqrt(max(var, 0.0) / n)
        mean, stderr = torch.tensor(mean, dtype=torch.float64), torch.tensor(stderr, dtype=torch.float64)
        filled = [float(s) for s, c in zip(sums[0].tolist(), count.tolist()) if c]
        loss = math.fsum(filled) / total if total and not any(math.isnan(s) for s in filled) else math.nan
        return {"count": count, "mean": mean, "stderr": stderr, "edges": self.edges(), "loss": loss, "rejected": rejected}

    def reset(self):
        """Zero the state on the current stream."""
        self.meter.zero_()
        self.counts.zero_()
        return self

    def _same_table(self, T, B, what):
        if (int(T), int(B)) != (self.num_timesteps, self.buckets):
            raise ValueError(f"{what}: (num_timesteps, buckets) = ({T}, {B}) does not match this meter's "
                             f"({self.num_timesteps}, {self.buckets})")

    def merge(self, other: "LossMeter"):
        """``self += other``, word by word on the int64 state: exactly the meter that saw both sets of images."""
        self._same_table(other.num_timesteps, other.buckets, "merge")
        self.meter += other.meter.to(self.meter.device)
        self.counts += other.counts.to(self.counts.device)
        return self

    def all_reduce(self, group=None):
        """``torch.distributed.all_reduce(SUM)`` of the int64 state: exact, so every rank ends with the same bits, those of one meter
        over all ranks' images.  A process without an initialised group keeps its state."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.meter, op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)
        return self

    def state_dict(self) -> Dict[str, object]:
        return {"num_timesteps": self.num_timesteps, "buckets": self.buckets, "meter": self.meter.detach().cpu().clone(),
                "counts": self.counts.detach().cpu().clone()}

    def load_state_dict(self, state: Dict[str, object]):
        self._same_table(state["num_timesteps"], state["buckets"], "load_state_dict")
        meter, counts = state["meter"], state["counts"]
        if tuple(meter.shape) != tuple(self.meter.shape) or tuple(counts.shape) != tuple(self.counts.shape) or \
                meter.dtype != torch.int64 or counts.dtype != torch.int64:
            raise ValueError("load_state_dict: the state tensors do not have this meter's shapes")
        self.meter.copy_(meter)
        self.counts.copy_(counts)
        return self


def validation_timesteps(idx: torch.Tensor, num_timesteps: int, t_offset: int = 0) -> torch.Tensor:
    """int64 ``t = ((((idx + t_offset) * 2654435761) & 0xFFFFFFFF) * num_timesteps) >> 32`` per dataset index: a multiplicative hash,
    so consecutive indices spread evenly over ``[0, num_timesteps)``.  The formula is a compatibility contract."""
    if torch.is_floating_point(idx):
        raise TypeError(f"dataset indices must be integers, got {idx.dtype}")
    h = ((idx.to(torch.int64) + _as_int64(t_offset)) * _HASH) & 0xFFFFFFFF          # (int64 wraps: the low 32 bits are the same)
    return (h * int(num_timesteps)) >> 32


@torch.no_grad()
def validation_loss(net, batches: Iterable, meter: LossMeter, base_seed: int = 0, t_offset: int = 0) -> LossMeter:
    """A validation pass that is a function of the checkpoint, the dataset, ``base_seed`` and ``t_offset`` -- in place of the body of
    ``validation_epoch`` (BaseRunner.py:214-249), whose ``net(x, x_cond)`` draws fresh ``t`` and noise at every call.

    ``batches`` yields ``(x, x_cond, idx)``; ``idx`` int64 ``[N]``: the dataset indices of the batch.  Per sample
    ``t = validation_timesteps(idx, T, t_offset)``, noise seed ``base_seed + idx``, ordinal 0.  ``x`` / ``x_cond`` are images, or -- on
    a latent model with an attached cache -- the int64 cache rows.  Runs under ``no_grad`` in ``eval()`` mode (restored afterwards),
    forms the context ``forward()`` forms and accumulates every image into ``meter``; no host read-back happens here
    (``meter.read()`` does that, after ``meter.all_reduce()`` under DDP).  Returns ``meter``."""
    was_training, meters = net.training, net._loss_meters
    dev = meter.device
    net.eval()
    net._loss_meters = (None, meter)
    try:
        for x, x_cond, idx in batches:
            idx = idx.reshape(-1)
            t = validation_timesteps(idx, net.num_timesteps, t_offset).to(dev)
            seeds = (idx.to(torch.int64) + _as_int64(base_seed)).to(dev)
            if not torch.is_floating_point(x):                               # rows of the attached latent cache
                net.p_losses_cached(x, x_cond, t, seeds=seeds, ordinals=0)
                continue
            x, x_cond = x.to(dev), x_cond.to(dev)
            if hasattr(net, "get_cond_stage_context"):                       # the latent model: LatentBrownianBridgeModel.forward
                context = net.get_cond_stage_context(x_cond)
                x, x_cond = net.encode(x, cond=False), net.encode(x_cond, cond=True)
            else:                                                            # BrownianBridgeModel.forward
                context = None if net.condition_key == "nocond" else x_cond
            net.p_losses(x, x_cond, context, t, seeds=seeds, ordinals=0)
    finally:
        net._loss_meters = meters
        net.train(was_training)
    return meter
