"""Latent cache for LBBDM training: encode the training set ONCE, gather the rows inside the q_sample kernel.

``LatentBrownianBridgeModel.forward`` (LatentBrownianBridgeModel.py:68-72) pushes both images of every pair through the frozen
VQGAN encoder on every micro-step of every epoch, and with ``normalize_latent`` the runner walks the training set twice more
through it for the four mean / std tensors (BBDMRunner.get_latent_mean_std, BBDMRunner.py:85-162).  The encoder is frozen and the
reference's datasets are deterministic per index (the flipped copy is an index of its own), so the latents of a training set are a
constant: computing them once is exact.

    cache = LatentCache.build(net, train_dataset, batch_size=32)      # or LatentCache.load(path, net)
    cache.install_stats(net)                                          # instead of get_latent_mean_std()
    net.attach_latent_cache(cache)
    loader = DataLoader(CachedPairs(train_dataset, names=cache.names), batch_size=..., shuffle=True)
    loss, log = net(x, x_cond)          # x, x_cond: the int64 [N] tensors the default collate makes of CachedPairs items

The rows are RAW latents (``encode(..., normalize=False)``); the normalisation, when configured, happens in the gather kernel from
the model's four attributes read at call time (``bbdm_bb_q_sample_cached_f32``, csrc/bridge.hip).  The statistics come from
``bbdm_latent_channel_stats_f32``.  Device-resident fp32 only: LBBDM-f4 is 2 x 3*64*64*4 B = 98 KB per pair.
"""
from __future__ import annotations

import hashlib
from typing import List, Optional, Sequence, Tuple

import torch
from torch.utils.data import DataLoader, Dataset

from .model import _launch, _need_gpu

_FORMAT = 1


def first_stage_fingerprint(model, M: int, latent_shape: Sequence[int]) -> str:
    """sha256 over what decides the cache's content: the first-stage ``state_dict`` tensors ``encode`` reads (``encoder.*`` and,
    unless ``latent_before_quant_conv``, ``quant_conv.*``: name, dtype, shape, bytes), that flag, ``M`` and the latent shape."""
    before = bool(model.model_config.latent_before_quant_conv)
    prefixes = ("encoder.",) if before else ("encoder.", "quant_conv.")
    h = hashlib.sha256()
    h.update(repr((_FORMAT, before, int(M), tuple(int(d) for d in latent_shape))).encode())
    for key, v in sorted(model.vqgan.state_dict().items()):
        if key.startswith(prefixes):
            v = v.detach().cpu().contiguous()
            h.update(repr((key, str(v.dtype), tuple(v.shape))).encode())
            h.update(v.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def channel_stats(z: torch.Tensor, row_blocks: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per-channel (mean, population variance, std) [C] of ``z`` [M, C, h, w] through ``bbdm_latent_channel_stats_f32``: the mean
    rounded once to fp32, the variance about that fp32 mean, sums in exact integer limbs -- a function of the multiset of rows
    (any row order, any ``row_blocks`` = blocks that share the rows, give the same bits)."""
    if z.dim() != 4 or z.dtype != torch.float32 or not z.is_contiguous():
        raise ValueError(f"channel_stats: a contiguous fp32 [M, C, h, w] tensor, got {tuple(z.shape)} {z.dtype}")
    _need_gpu(z)
    M, C, hw = z.shape[0], z.shape[1], z.shape[2] * z.shape[3]
    cells = torch.zeros(2 * C * 4, dtype=torch.float64, device=z.device)        # 2 x C exact limb cells (csrc/stats_acc.h)
    mean, var, std = (torch.empty(C, dtype=torch.float32, device=z.device) for _ in range(3))
    _launch(z, "bbdm_latent_channel_stats_f32", z.data_ptr(), M, C, hw, cells.data_ptr(), mean.data_ptr(), var.data_ptr(),
            std.data_ptr(), int(row_blocks))
    return mean, var, std


def _model_device(model) -> torch.device:
    return next(model.denoise_fn.parameters()).device


def _refuse_cond_stage(model):
    if model.cond_stage_model is not None:
        # a SpatialRescaler is trained and 'first_stage' conditions on the encoder's output of the pixels: both need the images
        raise ValueError(f"a latent cache cannot serve condition_key {model.condition_key!r}: its context is computed from the pixels "
                         "(the latent templates use 'nocond')")


class LatentCache:
    """Raw first-stage latents of a paired dataset: ``ori`` and ``cond`` [M, C, h, w] fp32 on the model's device, row i = item i;
    ``names`` the (name, cond name) of every item; ``fingerprint`` see :func:`first_stage_fingerprint`."""

    def __init__(self, ori: torch.Tensor, cond: torch.Tensor, names: List[Tuple[str, str]], fingerprint: str):
        self.ori, self.cond, self.names, self.fingerprint = ori, cond, names, fingerprint

    def __len__(self):
        return self.ori.shape[0]

    @classmethod
    @torch.no_grad()
    def build(cls, model, dataset, batch_size: int, num_workers: int = 0, verify: int = 8) -> "LatentCache":
        """Walk ``dataset`` in index order (items ``((x, name), (x_cond, name))``) through ``model.encode(..., normalize=False)``.
        ``verify``: that many evenly spaced items are fetched a second time and their pixels compared bitwise -- a dataset with random
        augmentation has no constant latents and raises ``ValueError``."""
        _refuse_cond_stage(model)
        M = len(dataset)
        if M == 0:
            raise ValueError("LatentCache.build: empty dataset")
        dev = _model_device(model)
        k = min(int(verify), M)
        probe = sorted({round(j * (M - 1) / max(k - 1, 1)) for j in range(k)})
        seen = {}
        ori = cond = None
        names: List[Tuple[str, str]] = []
        row = 0
        for (x, x_name), (x_cond, x_cond_name) in DataLoader(dataset, batch_size=batch_size, shuffle=False, drop_last=False,
                                                             num_workers=num_workers):
            n = x.shape[0]
            for i in probe:
                if row <= i < row + n:
                    seen[i] = (x[i - row].clone(), x_cond[i - row].clone())
            z = model.encode(x.to(dev), cond=False, normalize=False)
            zc = model.encode(x_cond.to(dev), cond=True, normalize=False)
            if ori is None:
                ori = torch.empty((M,) + tuple(z.shape[1:]), dtype=torch.float32, device=dev)
                cond = torch.empty_like(ori)
            ori[row:row + n] = z
            cond[row:row + n] = zc
            names += list(zip(x_name, x_cond_name))
            row += n
        if row != M:
            raise ValueError(f"LatentCache.build: the loader yielded {row} items of {M}")
        for i in probe:
            (x, _), (x_cond, _) = dataset[i]
            if not (torch.equal(torch.as_tensor(x), seen[i][0]) and torch.equal(torch.as_tensor(x_cond), seen[i][1])):
                raise ValueError(f"LatentCache.build: item {i} differs between two fetches (random augmentation?): "
                                 "the latents of this dataset are not a constant and cannot be cached")
        return cls(ori, cond, names, first_stage_fingerprint(model, M, ori.shape[1:]))

    def mean_std(self, row_blocks: int = 0):
        """(ori_mean, ori_std, cond_mean, cond_std), each [1, C, 1, 1] fp32 on the device -- what get_latent_mean_std computes with
        two more walks through the encoder (BBDMRunner.py:85-162), here two passes of :func:`channel_stats` over the cache."""
        out = []
        for z in (self.ori, self.cond):
            mean, _, std = channel_stats(z, row_blocks)
            out += [mean.view(1, -1, 1, 1), std.view(1, -1, 1, 1)]
        return tuple(out)

    def install_stats(self, model):
        """Assign the four attributes the runner's get_checkpoint_states saves (BBDMRunner.py:72-82)."""
        (model.ori_latent_mean, model.ori_latent_std, model.cond_latent_mean, model.cond_latent_std) = self.mean_std()

    def save(self, path):
        torch.save({"format": _FORMAT, "ori": self.ori.cpu(), "cond": self.cond.cpu(), "names": [list(p) for p in self.names],
                    "fingerprint": self.fingerprint}, path)

    @classmethod
    def load(cls, path, model) -> "LatentCache":
        """Read a :meth:`save` file onto ``model``'s device; ``ValueError`` when it was built by another first stage (or another
        ``latent_before_quant_conv``, size or shape)."""
        _refuse_cond_stage(model)
        rec = torch.load(path, map_location="cpu", weights_only=True)
        if rec.get("format") != _FORMAT:
            raise ValueError(f"{path}: not a latent cache of format {_FORMAT}")
        want = first_stage_fingerprint(model, rec["ori"].shape[0], rec["ori"].shape[1:])
        if rec["fingerprint"] != want:
            raise ValueError(f"{path}: fingerprint mismatch -- the cache was built by another first stage "
                             f"({rec['fingerprint'][:12]}.. != {want[:12]}..); rebuild it")
        dev = _model_device(model)
        return cls(rec["ori"].to(dev), rec["cond"].to(dev), [tuple(p) for p in rec["names"]], rec["fingerprint"])


class CachedPairs(Dataset):
    """``dataset``'s length and names with the images replaced by their index: item i is ``((i, name), (i, cond name))``, i an int64
    scalar, so the default collate hands the runner's ``loss_fn`` int64 [N] tensors where it expects images.  ``names``
    (``cache.names``) spares the fetch of item i -- two image decodes -- that reading the names from ``dataset`` costs."""

    def __init__(self, dataset, names: Optional[Sequence[Tuple[str, str]]] = None):
        if names is not None and len(names) != len(dataset):
            raise ValueError(f"CachedPairs: {len(names)} names for {len(dataset)} items")
        self.dataset, self.names = dataset, names

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        if self.names is not None:
            name, cond_name = self.names[i]
        else:
            (_, name), (_, cond_name) = self.dataset[i]
        idx = torch.tensor(i, dtype=torch.int64)
        return (idx, name), (idx, cond_name)
