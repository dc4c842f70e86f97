"""Continuous-batching bridge sampler: many sampling requests through ONE UNet plan of a fixed width, each image at its own step.

The reference samples a test set by calling ``net.sample(x_cond)`` ``sample_num`` times on every test batch
(runners/DiffusionBasedModelRunners/BBDMRunner.py:224-253): 200-step loops at batch 8, and a smaller batch at the end of the set.
``p_sample`` moves a whole batch through one shared step index, so such a batch can be neither widened nor topped up.  Here every slot
of a ``batch_size``-wide batch carries its own position in ``model.steps``:

* one UNet call per step with the slots' own timesteps (``UNetModel.infer_steps``: one plan, one hipGraph);
* one launch of ``bbdm_bb_p_sample_step_requests_f32`` (csrc/bridge.hip), the fused update of ``p_sample`` with a step, next step,
  flag, eta and clip decision per image -- bit for bit the scalar kernel's result for an image at the same (step, next, last, eta,
  clip);
* a request that finishes frees its slot, and the next queued request starts there at ``x_t = y`` (BrownianBridgeModel.py:203-221).

The reference fixes the step table (``sample_step`` / ``skip_sample`` / ``sample_type``, BrownianBridgeModel.py:69-79), ``eta`` (:195)
and ``clip_denoised`` per model or per call.  Here a request may carry its own :class:`SamplingParams`: a 20-step preview, a
deterministic ``eta = 0`` request and a clipped one share the batch -- and the plan and its hipGraph -- with 200-step requests.  A
slot holds its request's step table, a request finishes at the end of its own table, and the slot it frees is refilled at once.  A
request with params P computes what a model configured with P computes (``bridge_schedule`` builds both step tables).  Per step
the sampler uploads ONE int64 table of 4 rows of ``batch_size`` (step, next step, flag, eta; ``noise="philox"``: 6 rows, with seed
and ordinal): bit 2 of a flag says "clip this image", and the eta row holds the slots' ``batch_size`` fp32 values in its first half.

Noise contract: the noise of a request's k-th step with ``steps[i] != 0`` (``steps``: the request's own table) is
``torch.randn(shape, generator=its_generator, device=dev)`` drawn in step order, and nothing else draws from that generator.  The noise a request receives is therefore independent of its slot,
its batch-mates and its arrival time.  Its result still depends on its batch-mates through the fp16-pair bounds that the UNet plan takes
over the batch (within tolerance, not bitwise).  A group of requests submitted together and run in lockstep computes exactly what
``model.sample`` computes on the same conditions with the same noise.

``noise="philox"`` replaces that protocol by a formula: a request carries an ``int`` seed instead of a generator, and the noise of its
step at position i of ITS OWN step table is ``bbdm_amd.philox_normal(shape, [seed], [i])`` (csrc/philox.h; DESIGN.md "Seed-addressed
noise") -- a function of (seed, i, element) that needs no generator object, can be recomputed for one step alone, and is what
``model_P.sample(..., seeds=...)`` draws for the same seed, ``model_P`` being a model configured with the request's params (without
params: the sampler's model).  It is generated inside the bridge launch (``bbdm_bb_p_sample_step_requests_philox_f32``): a step
issues no ``normal_`` launch and the sampler holds no noise buffer; seeds and positions travel in the index tensor that a step
uploads anyway.
"""
from __future__ import annotations

import collections
import ctypes
import dataclasses
import math
import numbers
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .model import BrownianBridgeModel, LatentBrownianBridgeModel, _OBJECTIVES, _as_int64, _f32c, _launch, bridge_schedule
from .unet import UNetModel

_STEP, _LAST, _IDLE = 0, 1, 2          # per-slot state, bits 0-1 of the flag word of bbdm_bb_p_sample_step_requests_f32 ...
_CLIP = 4                              # ... and bit 2: clamp this image's x0_recon
_T, _T_NEXT, _FLAG, _ETA, _SEED, _ORDINAL = range(6)          # rows of the index table a step uploads


@dataclasses.dataclass(frozen=True)
class SamplingParams:
    """How ONE request is sampled, where the reference has one value per model.  ``None`` means the model's value (``clip_denoised``:
    the sampler's).  ``sample_step`` / ``skip_sample`` / ``sample_type`` give the request the step table of a model configured with
    them (BrownianBridgeModel.py:69-79, through ``bridge_schedule``); ``steps``, an explicit strictly descending sequence of
    timesteps ending in 0, overrides the three.  ``eta``: the factor of sigma_t (BrownianBridgeModel.py:195), a finite number >= 0."""
    sample_step: Optional[int] = None
    skip_sample: Optional[bool] = None
    sample_type: Optional[str] = None
    eta: Optional[float] = None
    clip_denoised: Optional[bool] = None
    steps: Optional[Sequence[int]] = None

    def __post_init__(self):
        if self.steps is not None:
            object.__setattr__(self, "steps", tuple(self.steps))          # immutable and hashable, like the other fields


class _Request:
    __slots__ = ("key", "y", "ctx", "gen", "steps", "eta", "clip")

    def __init__(self, key, y, ctx, gen, steps, eta, clip):
        self.key, self.y, self.ctx, self.gen, self.steps, self.eta, self.clip = key, y, ctx, gen, steps, eta, clip


def _pow2(k: int) -> int:
    p = 1
    while p < k:
        p *= 2
    return p


class BridgeSampler:
    """``BridgeSampler(model, batch_size, clip_denoised=False, noise="torch")`` for a :class:`BrownianBridgeModel` or
    :class:`LatentBrownianBridgeModel` in ``eval()``.  ``noise``: ``"torch"`` (a ``torch.Generator`` per request) or ``"philox"`` (an
    ``int`` seed per request; see the module docstring).

    ``submit([(key, x_cond, generator_or_seed), ...])`` queues a group of requests (``x_cond``: one condition image ``[C, H, W]``); iterating
    over the sampler runs steps until every queued request has finished and yields ``(key, sample)`` as each one does -- in pixel space
    (LBBDM: ``decode(latent, cond=False)``).  A request may be ``(key, x_cond, generator_or_seed, params)`` with a
    :class:`SamplingParams`: its own step table, eta and clip decision; without one it takes ``model.steps``, ``model.eta`` and the
    sampler's ``clip_denoised``.  ``sample_set`` is the ``sample_to_eval``-shaped helper.  All requests share one sample shape."""

    def __init__(self, model: BrownianBridgeModel, batch_size: int, clip_denoised: bool = False, noise: str = "torch"):
        if not isinstance(model, BrownianBridgeModel):
            raise TypeError("BridgeSampler drives a bbdm_amd BrownianBridgeModel / LatentBrownianBridgeModel")
        if not isinstance(model.denoise_fn, UNetModel):
            raise TypeError("BridgeSampler needs the bbdm_amd UNetModel as denoise_fn (per-image timesteps on its plan)")
        if model.objective not in _OBJECTIVES:
            raise NotImplementedError
        if int(batch_size) < 1 or int(batch_size) > 65535:
            raise ValueError(f"batch_size must be in [1, 65535], got {batch_size}")
        if noise not in ("torch", "philox"):
            raise ValueError(f"noise must be 'torch' or 'philox', got {noise!r}")
        self.philox = noise == "philox"
        self.model, self.width, self.clip = model, int(batch_size), bool(clip_denoised)
        self.latent = isinstance(model, LatentBrownianBridgeModel)
        self.device = model.m_t.device
        self._queue: collections.deque = collections.deque()
        self._slots: List[Optional[list]] = [None] * self.width        # [request, i] per slot: i = its position in request.steps
        self._shape = None              # (x_t shape per image, context shape per image or None)
        self._plan = None
        self._x = self._x_other = self._y = self._ctx = self._noise = self._x0 = None

    # ------------------------------------------------------------------------------------------------------
    def _check_schedule(self, steps):
        """The checks of ``p_sample`` (model.py) for every index a request with the step table ``steps`` will take, at submission."""
        m = self.model
        for i, step in enumerate(steps):
            nxt = 0 if step == 0 else steps[i + 1]
            if not (0 <= step < m.num_timesteps and 0 <= nxt < m.num_timesteps):
                raise IndexError(f"timestep {max(step, nxt)} is out of range for the {m.num_timesteps}-entry schedule")
        return steps

    def _resolve(self, params: Optional[SamplingParams]):
        """(step table, eta, clip) of a request, raising what building a model with these params, or stepping it, would raise."""
        m = self.model
        if params is None:
            return self._check_schedule(m._steps_host()), float(m.eta), self.clip
        if not isinstance(params, SamplingParams):
            raise TypeError(f"the fourth element of a request is a SamplingParams or None, got {type(params).__name__}")
        if params.steps is not None:
            steps = list(params.steps)
            if not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in steps):
                raise ValueError(f"steps must be integers, got {steps}")
            if not steps or steps[-1] != 0 or any(a <= b for a, b in zip(steps, steps[1:])):
                raise ValueError(f"steps must be strictly descending and end in 0 (and hold no other 0), got {steps}")
            steps = [int(v) for v in steps]
        elif params.sample_step is None and params.skip_sample is None and params.sample_type is None:
            steps = m._steps_host()
        else:
            skip = m.skip_sample if params.skip_sample is None else params.skip_sample
            stype = m.sample_type if params.sample_type is None else params.sample_type
            sstep = m.sample_step if params.sample_step is None else params.sample_step
            if skip and stype == "linear" and sstep < 3:
                raise ValueError(f"sample_step must be >= 3 with skip_sample and sample_type 'linear' (a stride of "
                                 f"(T - 1) / (sample_step - 2)), got {sstep}")
            steps = bridge_schedule(m.num_timesteps, m.mt_type, m.max_var, skip, stype, sstep)[1]
            if steps is None:                   # (the reference leaves self.steps unset for another sample_type)
                raise NotImplementedError(f"sample_type {stype!r}")
            steps = [int(v) for v in steps]
        eta = m.eta if params.eta is None else params.eta
        if params.eta is not None:
            ok = isinstance(eta, numbers.Real) and not isinstance(eta, bool) and math.isfinite(eta) and eta >= 0
            if not ok or not math.isfinite(ctypes.c_float(eta).value):          # the kernel takes it as fp32
                raise ValueError(f"eta must be a finite number >= 0, got {eta!r}")
        return self._check_schedule(steps), float(eta), self.clip if params.clip_denoised is None else bool(params.clip_denoised)

    def _condition(self, x_cond: torch.Tensor):
        """(y, context) of a batch of conditions, as ``p_sample_loop`` / ``LatentBrownianBridgeModel.sample`` form them."""
        m = self.model
        if self.latent:
            y = m.encode(x_cond, cond=True)
            ctx = m.get_cond_stage_context(x_cond)
        else:
            y, ctx = x_cond, None
        if m.condition_key == "nocond":
            ctx = None
        else:
            ctx = y if ctx is None else ctx
        return _f32c(y), None if ctx is None else _f32c(ctx)

    def submit(self, requests: Iterable[tuple]):
        """Queue a group of ``(key, x_cond, generator_or_seed)`` or ``(key, x_cond, generator_or_seed, params)``.  The group's distinct
        conditions go through the first stage and the conditioning stage in ONE call each.  Raises what ``p_sample`` raises for a
        condition of another shape (RuntimeError) or a schedule it would index out of range (IndexError), and what a model built with
        a request's params would raise (see :class:`SamplingParams`; ValueError / NotImplementedError), before anything is queued."""
        reqs = [tuple(r) for r in requests]
        if not reqs:
            return
        if any(len(r) not in (3, 4) for r in reqs):
            raise ValueError("a request is (key, x_cond, generator_or_seed) or (key, x_cond, generator_or_seed, params)")
        reqs = [r if len(r) == 4 else r + (None,) for r in reqs]
        for _, _, gen, _ in reqs:
            is_seed = isinstance(gen, numbers.Integral) and not isinstance(gen, bool)
            if self.philox and not is_seed:
                raise TypeError(f"noise='philox' takes an int seed per request, got {type(gen).__name__}")
            if not self.philox and is_seed:
                raise TypeError("noise='torch' takes a torch.Generator per request, got an int (seeds belong to noise='philox')")
        resolved = {}                  # one (step table, eta, clip) per distinct params of the group
        for _, _, _, p in reqs:
            if p not in resolved:
                resolved[p] = self._resolve(p)
        rows, uniq = [], {}
        for _, c, _, _ in reqs:          # requests that pass the same tensor object share its row (sample_set: sample_num draws per condition)
            if id(c) not in uniq:
                uniq[id(c)] = len(rows)
                rows.append(c if c.dim() == 3 else c.reshape(c.shape[-3:]))
        x_cond = torch.stack([r.to(self.device, torch.float32) for r in rows])
        with torch.no_grad():
            y, ctx = self._condition(x_cond)
        cin = y.shape[1] + (ctx.shape[1] if ctx is not None else 0)
        if cin != self.model.denoise_fn.in_channels:           # (UNetModel._check_inputs, where p_sample would fail)
            raise RuntimeError(f"expected {self.model.denoise_fn.in_channels} input channels (x + context), got {cin}")
        shape = (tuple(y.shape[1:]), None if ctx is None else tuple(ctx.shape[1:]))
        if self._shape is None:
            self._allocate(shape)
        elif shape != self._shape:
            raise RuntimeError(f"condition of shape {shape} in a sampler of shape {self._shape} (one sample shape per sampler)")
        for key, c, gen, p in reqs:
            r = uniq[id(c)]
            self._queue.append(_Request(key, y[r], None if ctx is None else ctx[r], _as_int64(gen) if self.philox else gen,
                                        *resolved[p]))

    def _allocate(self, shape):
        self._shape = shape
        W, f32 = self.width, dict(dtype=torch.float32, device=self.device)
        # zeros, not empty: the rows of idle slots still go through the UNet (their output is ignored), and must be finite there
        self._y = torch.zeros((W,) + shape[0], **f32)
        self._x = torch.zeros((W,) + shape[0], **f32)
        self._x_other = torch.zeros((W,) + shape[0], **f32)
        self._noise = None if self.philox else torch.zeros((W,) + shape[0], **f32)      # philox: the noise never touches memory
        self._x0 = torch.zeros((W,) + shape[0], **f32)
        self._ctx = None if shape[1] is None else torch.zeros((W,) + shape[1], **f32)

    # ------------------------------------------------------------------------------------------------------
    def busy(self) -> bool:
        return bool(self._queue) or any(s is not None for s in self._slots)

    def __iter__(self) -> Iterator[Tuple[object, torch.Tensor]]:
        while self.busy():
            yield from self.step()

    def _refill(self):
        """Free slots take the next queued requests, starting at x_t = y.  Only their rows are written: of the sampler's y / x_t /
        context and -- when the plan holds the sampler's tensors -- of the plan's input buffers, so the UNet call copies nothing."""
        free = [j for j, s in enumerate(self._slots) if s is None]
        if not free or not self._queue:
            return
        plan = self._plan
        held_x, held_c = plan.holding(self._x, self._ctx) if plan is not None else (False, False)
        for j in free:
            if not self._queue:
                break
            req = self._queue.popleft()
            self._slots[j] = [req, 0]
            self._y[j].copy_(req.y)
            self._x[j].copy_(req.y)
            if held_x:
                plan.x_in[j].copy_(req.y)
            if self._ctx is not None:
                self._ctx[j].copy_(req.ctx)
                if held_c:
                    plan.ctx_in[j].copy_(req.ctx)
        if held_x:
            plan.holds_input(self._x)
        if held_c and self._ctx is not None:
            plan.holds_context(self._ctx)

    @torch.no_grad()
    def step(self) -> List[Tuple[object, torch.Tensor]]:
        """One sampler step: refill, one UNet call, the noise of the slots that need it, one bridge launch; returns the requests that
        finished in it as ``(key, sample)``."""
        self._refill()
        live = [j for j, s in enumerate(self._slots) if s is not None]
        if not live:
            return []
        m, W = self.model, self.width
        # step, next step, flag and eta per slot (philox: ... and its seed and ordinal, its position in its step table): ONE upload.
        # The eta row holds the W fp32 values in its first 4 W bytes.
        tab = np.zeros((6 if self.philox else 4, W), dtype=np.int64)
        tab[_FLAG] = _IDLE
        eta = tab[_ETA].view(np.float32)
        noisy = []
        for j in live:
            req, i = self._slots[j]
            step = req.steps[i]
            tab[_T, j] = step
            if step == 0:
                tab[_FLAG, j] = _LAST | (_CLIP if req.clip else 0)
            else:
                tab[_T_NEXT, j], tab[_FLAG, j], eta[j] = req.steps[i + 1], _STEP | (_CLIP if req.clip else 0), req.eta
                noisy.append(j)
                if self.philox:
                    tab[_SEED, j], tab[_ORDINAL, j] = req.gen, i
        idx_d = torch.from_numpy(tab).to(self.device)
        pred, plan = m.denoise_fn.infer_steps(self._x, idx_d[_T], self._ctx)
        self._plan = plan
        x, xn = self._x, self._x_other
        if self.philox:                  # the noise is generated inside the launch: philox_normal(shape, seed, i) per slot
            _launch(x, "bbdm_bb_p_sample_step_requests_philox_f32", x.data_ptr(), self._y.data_ptr(), pred.data_ptr(),
                    idx_d[_SEED].data_ptr(), idx_d[_ORDINAL].data_ptr(), m.m_t.data_ptr(), m.variance_t.data_ptr(),
                    idx_d[_T].data_ptr(), idx_d[_T_NEXT].data_ptr(), idx_d[_FLAG].data_ptr(), idx_d[_ETA].data_ptr(),
                    _OBJECTIVES[m.objective], xn.data_ptr(), self._x0.data_ptr(), plan.x_in.data_ptr(), W, x[0].numel())
        else:
            for j in noisy:              # == torch.randn(shape, generator=gen, device=dev): randn is empty(...).normal_(0, 1, gen)
                self._noise[j].normal_(generator=self._slots[j][0].gen)
            _launch(x, "bbdm_bb_p_sample_step_requests_f32", x.data_ptr(), self._y.data_ptr(), pred.data_ptr(),
                    self._noise.data_ptr(), m.m_t.data_ptr(), m.variance_t.data_ptr(), idx_d[_T].data_ptr(),
                    idx_d[_T_NEXT].data_ptr(), idx_d[_FLAG].data_ptr(), idx_d[_ETA].data_ptr(), _OBJECTIVES[m.objective],
                    xn.data_ptr(), self._x0.data_ptr(), plan.x_in.data_ptr(), W, x[0].numel())
        plan.holds_input(xn)                        # x_in holds x_next (the kernel's second destination): the next call copies nothing
        self._x, self._x_other = xn, x
        done = []
        for j in live:
            slot = self._slots[j]
            if slot[1] == len(slot[0].steps) - 1:
                done.append(j)
            else:
                slot[1] += 1
        out = self._emit(done)
        for j in done:
            self._slots[j] = None
        return out

    def _emit(self, done: Sequence[int]) -> List[Tuple[object, torch.Tensor]]:
        if not done:
            return []
        keys = [self._slots[j][0].key for j in done]
        if not self.latent:
            imgs = torch.stack([self._x[j] for j in done])
        else:
            # ONE decode call for the slots that finished together, padded to a power of two with copies of its last row: a few plan
            # shapes for the first stage (a lockstep group of a power-of-two size decodes unpadded, as model.sample does)
            rows = list(done) + [done[-1]] * (_pow2(len(done)) - len(done))
            imgs = self.model.decode(torch.stack([self._x[j] for j in rows]), cond=False)[:len(done)]
        return list(zip(keys, imgs.unbind(0)))

    # ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_set(self, conds: torch.Tensor, sample_num: int, seeds: Sequence[int], group: int = 8,
                   params: Optional[SamplingParams] = None) -> torch.Tensor:
        """``sample_to_eval``'s sampling (BBDMRunner.py:224-253) over a whole test set: ``sample_num`` samples of each of the M
        conditions ``conds`` [M, C, H, W].  Each test batch of ``group`` conditions is submitted as one group; the sample (m, s) draws
        its noise from a generator on the model's device seeded with ``seeds[m * sample_num + s]`` (``noise="philox"``: that seed is
        the request's Philox key, passed straight through).  ``params``: one :class:`SamplingParams` for every request.  Returns
        [M, sample_num, C, H, W]."""
        M = conds.shape[0]
        seeds = [int(s) for s in torch.as_tensor(seeds).reshape(-1).tolist()]
        if len(seeds) != M * sample_num:
            raise ValueError(f"sample_set: {len(seeds)} seeds for {M} conditions x {sample_num} samples")
        for b0 in range(0, M, group):
            reqs = []
            for mi in range(b0, min(M, b0 + group)):
                c = conds[mi]
                for s in range(sample_num):
                    g = seeds[mi * sample_num + s]
                    if not self.philox:
                        g = torch.Generator(device=self.device)
                        g.manual_seed(seeds[mi * sample_num + s])
                    reqs.append(((mi, s), c, g, params))
            self.submit(reqs)
        out = None
        for (mi, s), img in self:
            if out is None:
                out = img.new_empty((M, sample_num) + tuple(img.shape))
            out[mi, s] = img
        return out
