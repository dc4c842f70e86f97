"""Evaluation metrics of a sample set, taken on the device from the uint8 images (``csrc/metrics.hip``).

The reference scores a checkpoint offline: ``preprocess_and_evaluation.py -f diversity`` -> ``evaluation/diversity.py:8-39`` re-opens
every PNG of ``sample_to_eval``'s result directory with PIL and forms the per-pixel standard deviation of the ``sample_num`` samples
of each condition with torch on the CPU; it has no paired metric (PSNR, SSIM, MAE against the ground truth) at all.  The quantity
that is evaluated is the uint8 image in the PNG file -- the bytes ``bbdm_images_to_u8_f32`` produces (:mod:`bbdm_amd.egress`) --
so here the same numbers come from the device tensors, before or without any file:

* :func:`pair_metrics`      -- per-image ``mae``, ``mse``, ``psnr``, ``ssim`` of a batch against its targets.
* :func:`diversity`         -- ``calc_diversity``'s number per condition and its mean.
* :class:`SetEvaluator`     -- the streaming form for a test set: feed targets and samples as they finish, read the means.
* :func:`metrics_from_dirs` -- the same kernels fed from the directory layout ``sample_to_eval`` / ``ImageWriter`` write.

Every function takes fp32 ``[N, C, H, W]`` device tensors (quantised first like the PNG writer, ``to_normal`` as there) or uint8
``[N, H, W, C]`` tensors (taken as they are).  The sums are exact integers or exact fixed-point limbs, so a result depends on the
bytes alone: metrics from tensors equal metrics from the written files, run after run.  No CPU fallback: the tensors live on the GPU.

LPIPS and FID (``evaluation/LPIPS.py``, ``evaluation/FID.py``) need the reference's external networks and stay with it.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import _lib
from .egress import _to_u8_device

__all__ = ["pair_metrics", "diversity", "SetEvaluator", "metrics_from_dirs", "ssim_window"]

_SA_W = 4                    # 64-bit words of one accumulator cell (csrc/stats_acc.h)
_WIN = 11


def ssim_window() -> Tuple[float, ...]:
    """The 11 weights ``exp(-(i - 5)^2 / (2 * 1.5^2))`` normalised by their fp64 sum (Wang et al. 2004: sigma = 1.5), built with
    ``math.exp`` on the host so that every back end gets the same eleven doubles."""
    g = [math.exp(-((i - _WIN // 2) ** 2) / (2.0 * 1.5 ** 2)) for i in range(_WIN)]
    s = math.fsum(g)
    return tuple(v / s for v in g)


_WINDOW = (ctypes.c_double * _WIN)(*ssim_window())


def _as_u8(images: torch.Tensor, to_normal: bool, lead: int = 1) -> torch.Tensor:
    """fp ``[*lead, C, H, W]`` -> quantised, or uint8 ``[*lead, H, W, C]`` as it is; returns contiguous uint8 ``[*lead, H, W, C]``."""
    if images.dim() != lead + 3:
        raise ValueError(f"expected {lead + 3} dimensions, got {tuple(images.shape)}")
    _lib.require_gpu(images)
    if images.dtype == torch.uint8:
        return images if images.is_contiguous() else images.contiguous()
    if not images.is_floating_point():
        raise TypeError(f"images are fp32 [.., C, H, W] or uint8 [.., H, W, C], got {images.dtype}")
    flat = images.reshape((-1,) + tuple(images.shape[lead:]))
    out = _to_u8_device(flat, to_normal)
    return out.reshape(tuple(images.shape[:lead]) + tuple(out.shape[1:]))


def _launch(t: torch.Tensor, name: str, *args):
    with _lib.device_guard(t.device):
        _lib.call(name, *args, _lib.current_stream(t.device))


def _check_pair(a: torch.Tensor, b: torch.Tensor):
    if a.shape != b.shape:
        raise ValueError(f"pred {tuple(a.shape)} and target {tuple(b.shape)} differ in shape")
    if a.device != b.device:
        raise ValueError("pred and target live on different devices")


def _pair_sums_raw(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """int64 [N, 2] = (sum |a - b|, sum (a - b)^2) of two uint8 [N, H, W, C] batches, on the device."""
    _check_pair(a, b)
    N, H, W, C = a.shape
    sums = torch.zeros(N, 2, dtype=torch.int64, device=a.device)
    _launch(a, "bbdm_u8_pair_sums", a.data_ptr(), b.data_ptr(), sums.data_ptr(), N, H, W, C)
    return sums


def _ssim_raw(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The SSIM accumulator cells int64 [N, 4] of two uint8 [N, H, W, C] batches, on the device."""
    _check_pair(a, b)
    N, H, W, C = a.shape
    cells = torch.zeros(N, _SA_W, dtype=torch.int64, device=a.device)
    _launch(a, "bbdm_u8_ssim", a.data_ptr(), b.data_ptr(), _WINDOW, cells.data_ptr(), N, H, W, C)
    return cells


def _read_cells(cells: torch.Tensor, name: str) -> torch.Tensor:
    out = torch.empty(cells.shape[0], dtype=torch.float64, device=cells.device)
    _launch(cells, name, cells.data_ptr(), out.data_ptr(), cells.shape[0])
    return out.cpu()


@torch.no_grad()
def pair_metrics(pred: torch.Tensor, target: torch.Tensor, to_normal: bool = True) -> Dict[str, torch.Tensor]:
    """Per-image ``mae``, ``mse``, ``psnr``, ``ssim`` (float64 host tensors [N]) of ``pred`` against ``target``, on the uint8 images.

    ``mae`` / ``mse``: the exact integer sums divided by H W C; ``psnr = 10 log10(255^2 / mse)`` (``inf`` for equal images); ``ssim``:
    Wang et al. 2004 per channel -- 11-tap Gaussian window (sigma 1.5), valid positions only, fp64 moments, C1 = (0.01 * 255)^2,
    C2 = (0.03 * 255)^2 -- averaged over the channels and the (H - 10)(W - 10) positions.  H, W >= 11."""
    a, b = _as_u8(pred, to_normal), _as_u8(target, to_normal)
    sums, cells = _pair_sums_raw(a, b), _ssim_raw(a, b)
    N, H, W, C = a.shape
    ssim_sum = _read_cells(cells, "bbdm_u8_ssim_read")
    sums = sums.cpu().to(torch.float64)
    count = float(H * W * C)
    mae, mse = sums[:, 0] / count, sums[:, 1] / count
    psnr = torch.tensor([10.0 * math.log10(65025.0 / v) if v > 0 else math.inf for v in mse.tolist()], dtype=torch.float64)
    return {"mae": mae, "mse": mse, "psnr": psnr, "ssim": ssim_sum / float(C * (H - (_WIN - 1)) * (W - (_WIN - 1)))}


def _diversity_raw(x: torch.Tensor) -> torch.Tensor:
    """The accumulator cells int64 [M, 4] of uint8 samples [M, S, H, W, C], on the device."""
    M, S, H, W, C = x.shape
    cells = torch.zeros(M, _SA_W, dtype=torch.int64, device=x.device)
    _launch(x, "bbdm_u8_diversity", x.data_ptr(), cells.data_ptr(), M, S, H, W, C)
    return cells


@torch.no_grad()
def diversity(samples: torch.Tensor, to_normal: bool = True) -> Tuple[torch.Tensor, float]:
    """``calc_diversity`` (evaluation/diversity.py:8-39) of ``samples``: fp32 ``[M, S, C, H, W]`` or uint8 ``[M, S, H, W, C]``, S samples
    of each of M conditions -> (per-condition float64 [M], their mean).  Per element the reference's fp32 sequence (mean over the
    samples, biased variance, square root); the standard deviations of a condition are summed exactly and divided by H W C in fp64,
    where the reference takes an fp32 ``torch.mean``."""
    x = _as_u8(samples, to_normal, lead=2)
    M, S, H, W, C = x.shape
    per = _read_cells(_diversity_raw(x), "bbdm_u8_diversity_read") / float(H * W * C)
    return per, float(per.mean())


class SetEvaluator:
    """Streaming evaluation of a test set: ``SetEvaluator(sample_num, to_normal=True)``.

    ``add_target(m, image)`` / ``add_sample(m, s, image)`` take one image (fp32 ``[C, H, W]`` or uint8 ``[H, W, C]``, on the device) of
    condition ``m`` and keep only its uint8 bytes there; ``consume`` drains an iterable of ``((m, s), image)`` -- what iterating a
    :class:`~bbdm_amd.BridgeSampler` yields after a ``sample_set``-style submission.  ``result()``: diversity = the mean over the
    conditions; psnr / ssim / mae = the means over all (m, s) of the conditions that have a target (the reference's ``calc_LPIPS``
    averages over ``total * num_samples`` the same way); conditions without a target count for the diversity only."""

    def __init__(self, sample_num: int, to_normal: bool = True):
        if int(sample_num) < 1:
            raise ValueError(f"sample_num must be >= 1, got {sample_num}")
        self.sample_num, self.to_normal = int(sample_num), bool(to_normal)
        self._targets: Dict[object, torch.Tensor] = {}
        self._samples: Dict[object, Dict[int, torch.Tensor]] = {}

    def _one(self, image: torch.Tensor) -> torch.Tensor:
        if image.dim() == 4 and image.shape[0] == 1:
            image = image[0]
        return _as_u8(image.unsqueeze(0), self.to_normal)[0].clone()

    @torch.no_grad()
    def add_target(self, m, image: torch.Tensor):
        self._targets[m] = self._one(image)

    @torch.no_grad()
    def add_sample(self, m, s: int, image: torch.Tensor):
        if not 0 <= int(s) < self.sample_num:
            raise ValueError(f"sample index {s} outside [0, {self.sample_num})")
        self._samples.setdefault(m, {})[int(s)] = self._one(image)

    def consume(self, results: Iterable[Tuple[Tuple[object, int], torch.Tensor]]):
        for (m, s), image in results:
            self.add_sample(m, s, image)
        return self

    @torch.no_grad()
    def result(self) -> Dict[str, object]:
        """``{"diversity", "psnr", "ssim", "mae"}`` (means, Python floats) plus ``"conditions"`` (their keys, in the order of the
        per-item arrays), ``"diversity_per_condition"`` [M] and ``"psnr_per_sample"`` / ``"ssim_per_sample"`` / ``"mae_per_sample"`` /
        ``"mse_per_sample"`` [conditions with a target, sample_num] with ``"paired_conditions"`` (their keys).  Raises ``ValueError``
        while a sample of any condition is missing, or a target has no samples."""
        conds = list(self._samples)
        if not conds:
            raise ValueError("no samples were added")
        for m in conds:
            missing = [s for s in range(self.sample_num) if s not in self._samples[m]]
            if missing:
                raise ValueError(f"condition {m!r}: samples {missing} of {self.sample_num} have not arrived")
        orphan = [m for m in self._targets if m not in self._samples]
        if orphan:
            raise ValueError(f"targets without samples: {orphan!r}")
        S = self.sample_num
        x = torch.stack([torch.stack([self._samples[m][s] for s in range(S)]) for m in conds])           # [M, S, H, W, C]
        per_div, div = diversity(x)
        out = {"conditions": conds, "diversity": div, "diversity_per_condition": per_div}
        paired = [m for m in conds if m in self._targets]
        out["paired_conditions"] = paired
        if paired:
            pred = torch.stack([self._samples[m][s] for m in paired for s in range(S)])
            target = torch.stack([self._targets[m] for m in paired for _ in range(S)])
            pm = pair_metrics(pred, target)
            for k in ("psnr", "ssim", "mae", "mse"):
                out[k + "_per_sample"] = pm[k].reshape(len(paired), S)
            for k in ("psnr", "ssim", "mae"):
                out[k] = float(pm[k].mean())
        else:
            for k in ("psnr", "ssim", "mae"):
                out[k] = math.nan
        return out


def _read_png(path: str, device) -> torch.Tensor:
    """The file's own pixels as uint8 [H, W, C] on ``device`` (PIL only decodes; a greyscale file has C = 1, as it was written)."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        a = np.array(im)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError(f"{path}: expected an 8-bit greyscale / RGB image, got {a.dtype} {a.shape}")
    return torch.from_numpy(a if a.ndim == 3 else a[:, :, None]).to(device)


def metrics_from_dirs(result_dir: str, gt_dir: Optional[str], num_samples: int, device="cuda") -> Dict[str, object]:
    """:class:`SetEvaluator`'s ``result()`` for the files ``sample_to_eval`` (BBDMRunner.py:224-253) writes: with ``num_samples > 1``
    ``result_dir/<name>/output_<j>.png`` (j < num_samples), with ``num_samples == 1`` ``result_dir/<name>.png``; the ground truth of
    ``<name>`` is ``gt_dir/<name>.png`` (``gt_dir=None``, or a missing file: that condition counts for the diversity only).  The
    conditions are taken in sorted order of their names."""
    ev = SetEvaluator(num_samples)
    device = torch.device(device)
    if num_samples > 1:
        names = sorted(d for d in os.listdir(result_dir) if os.path.isdir(os.path.join(result_dir, d)))
    else:
        names = sorted(os.path.splitext(f)[0] for f in os.listdir(result_dir) if f.endswith(".png"))
    for name in names:
        for j in range(num_samples):
            path = os.path.join(result_dir, name, f"output_{j}.png") if num_samples > 1 else os.path.join(result_dir, name + ".png")
            ev.add_sample(name, j, _read_png(path, device))
        gt = None if gt_dir is None else os.path.join(gt_dir, name + ".png")
        if gt is not None and os.path.exists(gt):
            ev.add_target(name, _read_png(gt, device))
    return ev.result()
