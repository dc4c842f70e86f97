"""Optimizer step + EMA update of the training loop as one HIP pass.

Drop-in mirrors of what the reference's runner builds around the model:

* :func:`get_optimizer`  -- ``runners/utils.py:48-57`` (``get_optimizer(optim_config, parameters)``): for ``'Adam'`` it
  returns :class:`FusedAdam`, a ``torch.optim.Optimizer`` with ``torch.optim.Adam``'s constructor, ``param_groups`` and
  ``state_dict()`` layout (``state[p] = {step, exp_avg, exp_avg_sq}``), so ``ReduceLROnPlateau`` (``BBDMRunner.py:61-66``)
  and the runner's optimizer checkpoints (``BaseRunner.py:128-151``) work unchanged; for ``'RMSProp'`` and ``'SGD'``, the
  other two values of the config schema, :class:`FusedRMSprop` and :class:`FusedSGD`, which mirror ``torch.optim.RMSprop``
  / ``torch.optim.SGD`` the same way (``bbdm_rmsprop_ema_step_f32`` / ``bbdm_sgd_ema_step_f32`` on the same chunk table).
* :class:`EMA`           -- ``runners/base/EMA.py:4-43``: same methods (``register / reset_device / update /
  apply_shadow / restore``) and the same ``shadow`` / ``backup`` dicts keyed by parameter name (the runner checkpoints
  ``ema.shadow`` directly, ``BaseRunner.py:125,169``).

Both hand the C-ABI entry ``bbdm_adam_ema_step_f32`` a device table of raw (param, grad, exp_avg, exp_avg_sq, shadow)
chunk pointers: ONE launch updates all 248 tensors.  When the EMA update is due in the same iteration the runner can fuse
it into the optimizer's pass with ``optimizer.step(ema=ema, ema_with_decay=...)``; called separately
(`ema.update(net)`, the unmodified runner) it is its own single pass.  No CPU / PyTorch fallback: parameters must be fp32
GPU tensors.

Beyond the reference (which never clips): ``FusedAdam / FusedSGD / FusedRMSprop(..., max_grad_norm=, skip_nonfinite=)`` --
global L2 gradient-norm clipping and a non-finite-gradient guard, computed on the device by two small launches over the same
chunk tables and applied INSIDE the update pass (no scale pass over the gradients, no host read-back); :func:`grad_norm` and
:func:`clip_grad_norm_` are the standalone forms (``torch.nn.utils.clip_grad_norm_``'s signature, norm type 2) for
optimizers torch provides.  The norm is summed in a fixed order and accumulated in exact integer limbs
(``csrc/stats_acc.h``): the same gradient values give the same bits on every run and on every rank.
``skip_nonfinite`` is also what answers a bad row index on the latent-cache path (``LatentBrownianBridgeModel.forward(indices)``,
bbdm_amd/latent_cache.py): indices that arrive on the CPU raise ``IndexError`` before any launch, but indices already on the
device are not read back, the gather kernel fills that image's rows with NaN, the loss and every gradient become NaN, and the
guard skips the step instead of writing them into the weights.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib

__all__ = ["FusedAdam", "FusedSGD", "FusedRMSprop", "EMA", "get_optimizer", "grad_norm", "clip_grad_norm_"]

_UNSET = object()


class _ChunkTable:
    """Device table of ``BbdmOptChunk`` entries, rebuilt only when one of the pointers it holds changes."""

    def __init__(self):
        self.key = None
        self.dev = None
        self.n = 0

    def get(self, rows, device):
        """rows: list of (param, grad|None, exp_avg|None, exp_avg_sq|None, shadow|None) tensors of equal numel."""
        key = tuple((p.data_ptr(), 0 if g is None else g.data_ptr(), 0 if m is None else m.data_ptr(),
                     0 if v is None else v.data_ptr(), 0 if s is None else s.data_ptr(), p.numel())
                    for p, g, m, v, s in rows)
        if key != self.key:
            ce = _lib.load().bbdm_opt_chunk_elems()
            ent = []
            for pp, gp, mp, vp, sp, n in key:
                for off in range(0, n, ce):
                    b = 4 * off
                    ent.append((pp + b, gp + b if gp else 0, mp + b if mp else 0, vp + b if vp else 0,
                                sp + b if sp else 0, min(ce, n - off)))
            host = torch.empty(len(ent), 6, dtype=torch.int64)
            for i, (a, b, c, d, e, n) in enumerate(ent):
                host[i, 0], host[i, 1], host[i, 2], host[i, 3], host[i, 4] = a, b, c, d, e
                host[i, 5] = n                        # int n + int pad: little-endian low word = n, high word = 0
            self.dev = host.to(device)
            self.key, self.n = key, len(ent)
        return self.dev, self.n


def _check_param(p: torch.Tensor):
    _lib.require_gpu(p)
    if p.dtype != torch.float32 or not p.is_contiguous():
        raise TypeError("bbdm_amd.optim works on contiguous fp32 parameters (the reference trains in fp32)")


def _launch(device, table, n, do_adam, group, step, ema_mode, ema_decay, clip=None, skip_nonfinite=False):
    """``clip`` (the 4-float device buffer :class:`_NormBuffers` ``.out``): the clipped entry point; None: the plain one."""
    args = (table.data_ptr(), n, int(do_adam), float(group["lr"]) if group else 0.0,
            float(group["betas"][0]) if group else 0.0, float(group["betas"][1]) if group else 0.0,
            float(group["eps"]) if group else 0.0, float(group["weight_decay"]) if group else 0.0,
            int(step), int(ema_mode), float(ema_decay))
    with _lib.device_guard(device):
        if clip is None:
            _lib.call("bbdm_adam_ema_step_f32", *args, _lib.current_stream(device))
        else:
            _lib.call("bbdm_adam_ema_step_clip_f32", *args, clip.data_ptr(), int(bool(skip_nonfinite)),
                      _lib.current_stream(device))


class _NormBuffers:
    """What the norm kernels write, owned here (the library never allocates): the limb cells of the squared norm (zeroed
    before each use), ``out`` = [norm, coef, ok, 0] fp32, and the int64 counter of skipped steps."""

    def __init__(self, device):
        self.cells = torch.zeros(_lib.load().bbdm_grad_norm_cells_bytes() // 8, dtype=torch.int64, device=device)
        self.out = torch.zeros(4, dtype=torch.float32, device=device)
        self.skipped = torch.zeros((), dtype=torch.int64, device=device)

    def run(self, device, tables, max_norm, count_skips):
        """One global norm over the gradients of ``tables`` [(device table, chunks)]: norm pass(es), then the finalize.
        ``max_norm`` None: coef = 1 (no clipping).  Nothing is read back."""
        self.cells.zero_()
        with _lib.device_guard(device):
            st = _lib.current_stream(device)
            for table, n in tables:
                _lib.call("bbdm_grad_sqnorm_f32", table.data_ptr(), n, self.cells.data_ptr(), st)
            _lib.call("bbdm_grad_norm_finalize_f32", self.cells.data_ptr(), float("inf") if max_norm is None else float(max_norm),
                      self.out.data_ptr(), self.skipped.data_ptr() if count_skips else None, st)


def _check_max_norm(max_norm):
    if max_norm is not None and not float(max_norm) >= 0.0:
        raise ValueError(f"max_grad_norm={max_norm}: must be >= 0 (or None: no clipping)")


class _FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: the chunk tables (one per parameter group, device and kind of step), the global gradient
    norm in front of the update (``max_grad_norm`` / ``skip_nonfinite``, attributes of the optimizer, not group entries), the fused
    ``ema=`` update and the EMA-only rows of parameters without a gradient.  A subclass supplies the rule:

    * ``_state_row(group, p)`` creates / advances ``state[p]`` as torch's class does and returns ``(kind, a, b)``: the tensors for the
      table's ``exp_avg`` and ``exp_avg_sq`` slots (None: unused by the rule) and whatever host-side value the launch depends on
      beyond the group's hyper-parameters (Adam: the step count; SGD: whether this step creates the momentum buffer).  Rows of one
      kind share one launch;
    * ``_launch_rule(device, table, n, group, kind, ema_mode, ema_decay, clip, skip_nonfinite)`` enqueues that launch."""

    def _init_fused(self, max_grad_norm, skip_nonfinite):
        _check_max_norm(max_grad_norm)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._tables: Dict[tuple, _ChunkTable] = {}
        self._norm: Optional[_NormBuffers] = None

    def _norm_buffers(self, device=None) -> _NormBuffers:
        if self._norm is None or (device is not None and self._norm.out.device != device):
            self._norm = _NormBuffers(device if device is not None else self.param_groups[0]["params"][0].device)
        return self._norm

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """Pre-clip global gradient norm of the last clipped / guarded step (None before the first one)."""
        return None if self._norm is None else self._norm.out[0]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """Number of steps the non-finite guard skipped: a 0-dim int64 DEVICE tensor (reading it is the caller's sync)."""
        return self._norm_buffers().skipped

    def _state_row(self, group, p):
        raise NotImplementedError

    def _launch_rule(self, device, table, n, group, kind, ema_mode, ema_decay, clip, skip_nonfinite):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None, ema: Optional["EMA"] = None, ema_with_decay: bool = True, max_grad_norm=_UNSET,
             skip_nonfinite=_UNSET):
        """One step of the optimizer's rule for every parameter that has a gradient.  ``ema`` (optional): also apply that EMA's
        update for these parameters in the same pass (``EMA.update(net, with_decay=ema_with_decay)`` semantics, on the updated
        weights).  ``max_grad_norm`` / ``skip_nonfinite``: override the optimizer's attributes for this call."""
        name = f"bbdm_amd.optim.{type(self).__name__}"
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        max_norm = self.max_grad_norm if max_grad_norm is _UNSET else max_grad_norm
        skip = self.skip_nonfinite if skip_nonfinite is _UNSET else bool(skip_nonfinite)
        _check_max_norm(max_norm)
        clipped = max_norm is not None or skip
        if clipped:                                   # ONE norm over every group: before any state is touched
            devices = {p.device for group in self.param_groups for p in group["params"] if p.grad is not None}
            if len(devices) > 1:
                raise ValueError(f"{name}: max_grad_norm / skip_nonfinite need every parameter that has a "
                                 f"gradient on ONE device (the norm is global); got {sorted(map(str, devices))}")
        launches = []                                 # (device, table, chunks, update?, group, kind, ema mode, decay, rows)
        for gi, group in enumerate(self.param_groups):
            kinds: Dict[tuple, list] = {}        # (device, kind) -> rows; normally ONE kind = one launch
            no_grad_rows = []                    # parameters without a gradient: no update (as torch) -- but EMA.update covers
            for p in group["params"]:           # EVERY registered parameter (EMA.py:21-29), so the fused pass does too
                if p.grad is None:
                    shadow = ema._shadow_of(p) if ema is not None else None
                    if shadow is not None:
                        _check_param(p)
                        no_grad_rows.append((p, None, None, None, shadow))
                    continue
                _check_param(p)
                g = p.grad
                if g.is_sparse or g.dtype != torch.float32:
                    raise RuntimeError(f"{name} needs dense fp32 gradients")
                if not g.is_contiguous():
                    g = p.grad = g.contiguous()
                kind, m, v = self._state_row(group, p)
                shadow = ema._shadow_of(p) if ema is not None else None
                kinds.setdefault((p.device, kind), []).append((p, g, m, v, shadow))
            mode = 0 if ema is None else (1 if ema_with_decay else 2)
            by_dev: Dict[torch.device, list] = {}
            for r in no_grad_rows:
                by_dev.setdefault(r[0].device, []).append(r)
            for device, rows in by_dev.items():
                table, n = self._tables.setdefault((gi, device, "ema-only"), _ChunkTable()).get(rows, device)
                launches.append((device, table, n, False, None, 0, mode, ema.ema_decay, rows))
            for (device, kind), rows in kinds.items():
                table, n = self._tables.setdefault((gi, device, len(kinds) > 1 and kind), _ChunkTable()).get(rows, device)
                launches.append((device, table, n, True, group, kind, mode, ema.ema_decay if ema is not None else 0.0, rows))
        clip = None
        if clipped:                                   # norm pass over the tables the update launches are about to use, then the finalize
            upd = [l for l in launches if l[3]]
            device = upd[0][0] if upd else self.param_groups[0]["params"][0].device
            norm = self._norm_buffers(device)
            norm.run(device, [(l[1], l[2]) for l in upd], max_norm, skip)
            clip = norm.out
        for device, table, n, update, group, kind, mode, decay, rows in launches:
            if update:
                self._launch_rule(device, table, n, group, kind, mode, decay, clip, skip)
                # the kernel rewrote the parameters behind autograd's back: bump their version counters, as an in-place torch op
                # would -- the UNet keys its packed weight copies (and autograd its saved-tensor checks) on them.  Without this the
                # next forward ran on the conv weights of BEFORE the step.
                torch.autograd.graph.increment_version([r[0] for r in rows])
            else:                                     # EMA only: the Adam entry with do_adam = 0, whatever the rule
                _launch(device, table, n, False, None, 0, mode, decay)
        return loss


class FusedAdam(_FusedOptimizer):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (no amsgrad / maximize) with the whole ``step()`` as
    one launch.  State layout = torch's: ``state[p]['step']`` (a float32 scalar tensor on the CPU, as torch keeps it for
    non-capturable Adam), ``'exp_avg'``, ``'exp_avg_sq'`` -- an optimizer checkpoint written by either loads into the
    other.

    ``max_grad_norm`` (None: off): ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` over ALL parameters of ALL groups that
    have a gradient (one global L2 norm), folded into the step: a norm pass and a one-workgroup finalize in front of the Adam
    launch, which multiplies each gradient by ``min(1, max_grad_norm / (norm + 1e-6))`` as it reads it (``p.grad`` itself is
    NOT rescaled).  ``skip_nonfinite``: when the norm is not finite (an Inf / NaN gradient, or a 16 384-element chunk whose norm
    exceeds 65 536: the accumulator's window, csrc/optim.hip) the parameters and both moments stay untouched; a fused ``ema=``
    update still happens, as the runner's ``ema.update`` would; ``skipped_steps`` counts these steps on the device.  Nothing on
    the host knows about a skip -- no read-back, no sync -- so the host-side ``state[p]['step']`` (and with it the bias
    correction of later steps) ADVANCES on a skipped step too.  Without ``skip_nonfinite`` a non-finite norm gives a NaN
    coefficient and NaN parameters (every parameter, where torch's Inf norm -> coef 0 spoils only the elements whose gradient was
    non-finite).  Both options are attributes of the optimizer, not entries of ``param_groups`` / ``defaults``: ``state_dict()``
    keeps torch's layout.  All parameters with a gradient must then live on one device (``ValueError`` otherwise).  With both
    off, ``step()`` is what it was: one ``bbdm_adam_ema_step_f32`` launch.

    ``grad_norm``: the pre-clip global norm of the last clipped / guarded step, a 0-dim fp32 device tensor (a view of the
    optimizer's buffer: the next such step overwrites it; ``.clone()`` to keep it).  NaN where ``skip_nonfinite`` skipped."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, max_grad_norm=None,
                 skip_nonfinite=False):
        if amsgrad:
            raise NotImplementedError("bbdm_amd.optim.FusedAdam: amsgrad is not implemented (the reference never sets it)")
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or weight_decay < 0.0:
            raise ValueError(f"invalid Adam hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=False, differentiable=False, fused=None))
        self._init_fused(max_grad_norm, skip_nonfinite)

    def _state_row(self, group, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["step"] += 1
        return int(st["step"]), st["exp_avg"], st["exp_avg_sq"]         # kind = the step count (the bias corrections)

    def _launch_rule(self, device, table, n, group, kind, ema_mode, ema_decay, clip, skip_nonfinite):
        _launch(device, table, n, True, group, kind, ema_mode, ema_decay, clip, skip_nonfinite)


def _call_rule(device, entry, args, clip, skip_nonfinite):
    """``entry`` + ``_f32`` (plain) or ``_clip_f32`` (``clip`` = the 4-float device buffer of :class:`_NormBuffers`)."""
    with _lib.device_guard(device):
        if clip is None:
            _lib.call(entry + "_f32", *args, _lib.current_stream(device))
        else:
            _lib.call(entry + "_clip_f32", *args, clip.data_ptr(), int(bool(skip_nonfinite)), _lib.current_stream(device))


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov)`` (no maximize) with the whole ``step()`` as one
    launch (``bbdm_sgd_ema_step_f32``); what :func:`get_optimizer` returns for ``'SGD'`` (``runners/utils.py:54-55``: momentum 0.9).
    State layout = torch's: ``state[p]['momentum_buffer']`` when momentum != 0, no state otherwise -- an optimizer checkpoint written
    by either class loads into the other.

    ``max_grad_norm``, ``skip_nonfinite``, ``grad_norm``, ``skipped_steps`` and ``step(ema=, ema_with_decay=)`` are
    :class:`FusedAdam`'s, to the letter: attributes of the optimizer, one global norm, the gradient scaled as the pass reads it.
    Nothing on the host knows about a skipped step.  The one place that shows: the step that creates a momentum buffer writes
    ``buf = grad`` (torch: ``clone(grad)``) where later steps apply ``buf = momentum * buf + (1 - dampening) * grad``; when
    ``skip_nonfinite`` skips that FIRST step the buffer stays at zero on the device, and the next step -- for the host no longer
    the first -- applies the recurrence to it: ``buf = (1 - dampening) * grad``, which differs from torch's ``buf = grad`` only
    when dampening != 0."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm=None,
                 skip_nonfinite=False):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"invalid SGD hyper-parameters lr={lr} momentum={momentum} weight_decay={weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=False, foreach=None, differentiable=False, fused=None))
        self._init_fused(max_grad_norm, skip_nonfinite)

    def _state_row(self, group, p):
        if group["momentum"] == 0:                    # no state at all, as in torch
            return "run", None, None
        st = self.state[p]
        buf = st.get("momentum_buffer")
        if buf is None:                               # torch: buf = clone(grad); here the kernel writes it (kind "first")
            buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            return "first", buf, None
        return "run", buf, None

    def _launch_rule(self, device, table, n, group, kind, ema_mode, ema_decay, clip, skip_nonfinite):
        _call_rule(device, "bbdm_sgd_ema_step",
                   (table.data_ptr(), n, float(group["lr"]), float(group["momentum"]), float(group["dampening"]),
                    float(group["weight_decay"]), int(bool(group["nesterov"])), int(kind == "first"), int(ema_mode),
                    float(ema_decay)), clip, skip_nonfinite)


class FusedRMSprop(_FusedOptimizer):
    """``torch.optim.RMSprop(params, lr, alpha, eps, weight_decay, momentum)`` (not centered, no maximize) with the whole ``step()``
    as one launch (``bbdm_rmsprop_ema_step_f32``); what :func:`get_optimizer` returns for ``'RMSProp'`` (``runners/utils.py:52-53``).
    State layout = torch's: ``state[p]['step']`` (a float32 scalar tensor on the CPU), ``'square_avg'`` and, when momentum > 0,
    ``'momentum_buffer'`` -- an optimizer checkpoint written by either class loads into the other.  ``centered=True`` needs a third
    state tensor (``grad_avg``) the chunk table has no slot for: ``NotImplementedError``, also for a checkpoint that carries one.

    ``max_grad_norm``, ``skip_nonfinite``, ``grad_norm``, ``skipped_steps`` and ``step(ema=, ema_with_decay=)`` are
    :class:`FusedAdam`'s, to the letter.  Nothing on the host knows about a skipped step, so ``state[p]['step']`` ADVANCES on a
    skipped step too; the rule has no bias correction, so that count is all that differs from an optimizer that never saw the
    step."""

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, max_grad_norm=None,
                 skip_nonfinite=False):
        if centered:
            raise NotImplementedError("bbdm_amd.optim.FusedRMSprop: centered is not implemented (the reference never sets it)")
        if lr < 0.0 or eps < 0.0 or momentum < 0.0 or weight_decay < 0.0 or alpha < 0.0:
            raise ValueError(f"invalid RMSprop hyper-parameters lr={lr} alpha={alpha} eps={eps} weight_decay={weight_decay} "
                             f"momentum={momentum}")
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=False, weight_decay=weight_decay,
                                      capturable=False, foreach=None, maximize=False, differentiable=False))
        self._init_fused(max_grad_norm, skip_nonfinite)

    _CENTERED = "bbdm_amd.optim.FusedRMSprop: a centered RMSprop checkpoint (grad_avg) cannot be loaded: centered is not implemented"

    def load_state_dict(self, state_dict):
        if any(g.get("centered") for g in state_dict["param_groups"]) or \
                any("grad_avg" in s for s in state_dict["state"].values()):
            raise NotImplementedError(self._CENTERED)
        super().load_state_dict(state_dict)

    def _state_row(self, group, p):
        st = self.state[p]
        if group.get("centered") or "grad_avg" in st:
            raise NotImplementedError(self._CENTERED)
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["square_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        buf = None
        if group["momentum"] > 0:
            buf = st.get("momentum_buffer")
            if buf is None:
                buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["step"] += 1
        return 0, buf, st["square_avg"]

    def _launch_rule(self, device, table, n, group, kind, ema_mode, ema_decay, clip, skip_nonfinite):
        _call_rule(device, "bbdm_rmsprop_ema_step",
                   (table.data_ptr(), n, float(group["lr"]), float(group["alpha"]), float(group["eps"]),
                    float(group["weight_decay"]), float(group["momentum"]), int(ema_mode), float(ema_decay)), clip, skip_nonfinite)


class EMA:
    """``runners/base/EMA.py`` with the update as one launch over all parameters."""

    def __init__(self, ema_decay):
        super().__init__()
        self.ema_decay = ema_decay
        self.backup = {}
        self.shadow = {}
        self._table = _ChunkTable()
        self._by_param: Dict[int, str] = {}

    def register(self, current_model: nn.Module):
        for name, param in current_model.named_parameters():
            if param.requires_grad:
                self.shadow[name] = param.data.clone()
                self._by_param[id(param)] = name

    def reset_device(self, current_model: nn.Module):
        for name, param in current_model.named_parameters():
            if param.requires_grad:
                self.shadow[name] = self.shadow[name].to(param.data.device)
                self._by_param[id(param)] = name

    def _shadow_of(self, param) -> Optional[torch.Tensor]:
        name = self._by_param.get(id(param))
        return None if name is None else self.shadow.get(name)

    @torch.no_grad()
    def update(self, current_model: nn.Module, with_decay=True):
        rows, device = [], None
        for name, param in current_model.named_parameters():
            if param.requires_grad:
                assert name in self.shadow
                _check_param(param)
                sh = self.shadow[name]
                if sh.data_ptr() == param.data_ptr():
                    raise RuntimeError("EMA.update() between apply_shadow() and restore(): the weights ARE the shadow")
                if sh.device != param.device or sh.dtype != torch.float32 or not sh.is_contiguous():
                    sh = self.shadow[name] = sh.to(device=param.device, dtype=torch.float32).contiguous()
                self._by_param[id(param)] = name
                device = param.device
                rows.append((param, None, None, None, sh))
        if not rows:
            return
        table, n = self._table.get(rows, device)
        _launch(device, table, n, False, None, 0, 1 if with_decay else 2, self.ema_decay)

    def apply_shadow(self, current_model: nn.Module):
        for name, param in current_model.named_parameters():
            if param.requires_grad:
                assert name in self.shadow
                self.backup[name] = param.data
                param.data = self.shadow[name]

    def restore(self, current_model: nn.Module):
        for name, param in current_model.named_parameters():
            if param.requires_grad:
                assert name in self.backup
                param.data = self.backup[name]
        self.backup = {}


_norm_tables: Dict[torch.device, _ChunkTable] = {}        # grad_norm / clip_grad_norm_: one cached table per device


def _global_grad_norm(parameters, max_norm, norm_type):
    """-> ([norm, coef, ok, 0] device buffer, function that applies ``grad *= coef``)."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"bbdm_amd.optim: only the L2 norm (norm_type=2) is implemented, got norm_type={norm_type}")
    _check_max_norm(max_norm)
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]          # as torch: a parameter without a gradient is left out
    if not grads:
        return torch.zeros(4), lambda: None
    device = grads[0].device
    for g in grads:
        if g.device != device:
            raise ValueError(f"bbdm_amd.optim: the gradients must live on one device, got {device} and {g.device}")
        _lib.require_gpu(g)
        if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous():
            raise TypeError("bbdm_amd.optim: the gradient norm works on dense contiguous fp32 gradients")
    table, n = _norm_tables.setdefault(device, _ChunkTable()).get([(g, g, None, None, None) for g in grads], device)
    norm = _NormBuffers(device)                   # fresh per call: the returned norm is the caller's to keep
    norm.run(device, [(table, n)], max_norm, False)

    def scale():
        with _lib.device_guard(device):
            _lib.call("bbdm_grad_scale_f32", table.data_ptr(), n, norm.out.data_ptr(), _lib.current_stream(device))
        torch.autograd.graph.increment_version(grads)
    return norm.out, scale


@torch.no_grad()
def grad_norm(parameters, norm_type: float = 2.0) -> torch.Tensor:
    """Global L2 norm of the gradients of ``parameters`` (a tensor or an iterable), a 0-dim fp32 tensor on their device: what
    ``torch.nn.utils.clip_grad_norm_`` returns, without the clipping, a host read-back or an order-dependent sum (NaN where the
    sum leaves the accumulator's window or a gradient is not finite: csrc/optim.hip)."""
    return _global_grad_norm(parameters, None, norm_type)[0][0]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False,
                    foreach: Optional[bool] = None) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` (norm type 2 only) in three launches: gradients *= min(1, max_norm / (norm + 1e-6)) in
    place; returns the norm before clipping.  For optimizers that are torch's own (the fused ones clip inside their own pass:
    ``max_grad_norm=``).  ``error_if_nonfinite`` reads the norm back (the one host sync here); ``foreach`` is accepted
    and ignored."""
    out, scale = _global_grad_norm(parameters, max_norm, norm_type)
    if error_if_nonfinite and not bool(torch.isfinite(out[0])):
        raise RuntimeError("bbdm_amd.optim.clip_grad_norm_: the total norm of the gradients is non-finite, so it cannot be "
                           "clipped (error_if_nonfinite=True)")
    scale()
    return out[0]


def get_optimizer(optim_config, parameters):
    """runners/utils.py:48-57 with every optimizer of the config schema on the device path: ``'Adam'`` -> :class:`FusedAdam`,
    ``'RMSProp'`` -> :class:`FusedRMSprop`, ``'SGD'`` -> :class:`FusedSGD` (momentum 0.9), with the reference's hyper-parameters.
    Two optional keys beyond the reference's yaml, honoured by all three: ``max_grad_norm`` and ``skip_nonfinite`` (absent = off,
    the reference's behaviour).  An unknown name raises ``NotImplementedError`` (the reference RETURNS the exception object, and
    the runner fails later on an unrelated attribute)."""
    extra = dict(max_grad_norm=getattr(optim_config, "max_grad_norm", None),
                 skip_nonfinite=getattr(optim_config, "skip_nonfinite", False))
    if optim_config.optimizer == 'Adam':
        return FusedAdam(parameters, lr=optim_config.lr, weight_decay=optim_config.weight_decay,
                         betas=(optim_config.beta1, 0.999), **extra)
    elif optim_config.optimizer == 'RMSProp':
        return FusedRMSprop(parameters, lr=optim_config.lr, weight_decay=optim_config.weight_decay, **extra)
    elif optim_config.optimizer == 'SGD':
        return FusedSGD(parameters, lr=optim_config.lr, momentum=0.9, **extra)
    else:
        raise NotImplementedError('Optimizer {} not understood.'.format(optim_config.optimizer))
