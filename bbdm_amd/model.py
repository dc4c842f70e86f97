"""BrownianBridgeModel / LatentBrownianBridgeModel -- drop-in mirrors of the reference classes, MI355X-native.

Reference: model/BrownianBridge/BrownianBridgeModel.py:15-225 and LatentBrownianBridgeModel.py:19-147.
The runner (runners/DiffusionBasedModelRunners/BBDMRunner.py:21-29, 164-253) touches the model only through
``Model(config.model)``, ``.apply(weights_init)``, ``.get_parameters()``, ``net(x, x_cond) -> (loss, dict)``,
``.sample(...)``, ``.encode(...)``, ``state_dict()/load_state_dict()`` and ``named_parameters()`` -- all kept with
the same names, argument meaning and error behaviour (asserts / NotImplementedError at the same places).

What changed underneath: ``denoise_fn`` is :class:`bbdm_amd.unet.UNetModel` (HIP kernels), and the scheduler
arithmetic (q_sample / predict_x0 / the p_sample update / the loss) are fused HIP kernels reached through the
C-ABI of ``include/bbdm_hip.h``.  Random numbers come from torch's generator by default (``torch.randn_like`` /
``torch.randint``), so ``main.py``'s seeding (main.py:57-65) keeps its meaning.  With ``seeds=`` the noise is generated on the
device inside the fused kernels instead, as a function of (seed, ordinal, element) -- :func:`philox_normal`, DESIGN.md
"Seed-addressed noise".  No CPU fallback exists.
"""
from __future__ import annotations

import itertools
import numbers
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .unet import UNetModel

try:                                   # tqdm is what the reference wraps its loops in; optional here
    from tqdm.autonotebook import tqdm
except Exception:                      # pragma: no cover
    def tqdm(it, **kw):
        return it

_OBJECTIVES = {"grad": 0, "noise": 1, "ysubx": 2}
_LOSSES = {"l1": 0, "l2": 1}


def _need_gpu(*ts):
    _lib.require_gpu(*ts)


def _launch(t: torch.Tensor, name: str, *args):
    """One C-ABI call on ``t``'s device and torch's current stream there."""
    with _lib.device_guard(t.device):
        _lib.call(name, *args, _lib.current_stream(t.device))


def _f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


NOISE_P_SAMPLE, NOISE_Q_SAMPLE = 0, 1          # the `domain` word of the noise counter (csrc/philox.h)


def _as_int64(v: int) -> int:
    """A Python integer as the int64 with the same low 64 bits (seeds are 64-bit keys: 2**63 .. 2**64 - 1 wrap)."""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def _i64_per_image(v, n, device, what):
    """``v`` (int64 tensor, sequence of ints or one int for all) as a contiguous int64 tensor [n] on ``device``."""
    if isinstance(v, torch.Tensor):
        if v.dtype != torch.int64:
            raise TypeError(f"{what} must be an int64 tensor or a sequence of ints, got a {v.dtype} tensor")
        out = v.reshape(-1).to(device).contiguous()
    else:
        vals = [v] * n if isinstance(v, numbers.Integral) else list(v)
        out = torch.tensor([_as_int64(x) for x in vals], dtype=torch.int64).to(device)
    if out.numel() != n:
        raise ValueError(f"{what}: {out.numel()} values for {n} images")
    return out


def philox_normal(shape_per_image, seeds, ordinals, domain=NOISE_P_SAMPLE, device=None):
    """Seed-addressed standard normals ``[N, *shape_per_image]`` (fp32): image n is a function of ``(seeds[n], ordinals[n],
    domain)`` alone -- Philox4x32-10 keyed by the seed, counter = (element / 4, ordinal, domain), Box-Muller on the four output
    words (csrc/philox.h; the layout is a compatibility contract).  These are the bits the fused kernels consume when
    ``p_sample`` / ``BridgeSampler`` / ``q_sample`` are given seeds: ``domain`` 0 is the noise of ``p_sample`` at
    ``ordinal = i`` (the position in ``model.steps``), 1 the noise of ``q_sample``.  ``seeds``: int64 tensor or sequence of ints
    (its length is N); ``ordinals``: the same, or one int for all images.  ``device``: defaults to the seeds' device when they
    are a tensor, else the current GPU."""
    shape = tuple(int(d) for d in shape_per_image)
    if device is None:
        device = seeds.device if isinstance(seeds, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    n = seeds.numel() if isinstance(seeds, torch.Tensor) else len(seeds)
    sd = _i64_per_image(seeds, n, device, "seeds")
    od = _i64_per_image(ordinals, n, device, "ordinals")
    out = torch.empty((n,) + shape, dtype=torch.float32, device=device)
    _need_gpu(out)
    if n and out[0].numel():
        _launch(out, "bbdm_philox_normal_f32", out.data_ptr(), sd.data_ptr(), od.data_ptr(), int(domain), n, out[0].numel())
    return out


def bridge_schedule(T, mt_type, max_var, skip_sample, sample_type, sample_step):
    """The six [T] schedule tables (float64 numpy, in registration order) and the sampling step table.

    m_t: 'linear' = linspace(0.001, 0.999); 'sin' = 1.0075**linspace(0, T) normalised with the last entry pinned to
    0.999.  variance_t = 2 (m_t - m_t^2) max_var.  The "*_tminus" tables are the same shifted by one step with a
    leading 0.  (BrownianBridgeModel.py:45-59; only m_t and variance_t are read by the sampler.)
    Step table (BrownianBridgeModel.py:69-79): skip+'linear' = arange(T-1, 1, -(T-1)/(sample_step-2)).long() ++ [1, 0];
    skip+'cosine' as the reference defines it (float64 values); no skip = T-1 .. 0.
    """
    if mt_type == "linear":
        m = np.linspace(0.001, 0.999, T)
    elif mt_type == "sin":
        m = np.power(1.0075, np.linspace(0, T, T))
        m /= m[-1]
        m[-1] = 0.999
    else:
        raise NotImplementedError
    shift = lambda a, first: np.concatenate(([first], a[:-1]))
    m_prev = shift(m, 0)
    var = 2. * (m - m ** 2) * max_var
    var_prev = shift(var, 0.)
    var_t_prev = var - var_prev * ((1. - m) / (1. - m_prev)) ** 2
    tables = {
        "m_t": m, "m_tminus": m_prev, "variance_t": var, "variance_tminus": var_prev,
        "variance_t_tminus": var_t_prev, "posterior_variance_t": var_t_prev * var_prev / var,
    }
    steps = None
    if not skip_sample:
        steps = torch.arange(T - 1, -1, -1)
    elif sample_type == "linear":
        stride = (T - 1) / (sample_step - 2)
        steps = torch.cat((torch.arange(T - 1, 1, step=-stride).long(), torch.tensor([1, 0], dtype=torch.long)))
    elif sample_type == "cosine":
        grid = np.linspace(start=0, stop=T, num=sample_step + 1)
        steps = torch.from_numpy((np.cos(grid / T * np.pi) + 1.) / 2. * T)
    return tables, steps


class BrownianBridgeModel(nn.Module):
    """BrownianBridgeModel.py:15-225."""

    def __init__(self, model_config):
        super().__init__()
        self.model_config = model_config
        model_params = model_config.BB.params
        self.num_timesteps = model_params.num_timesteps
        self.mt_type = model_params.mt_type
        self.max_var = model_params.max_var if model_params.__contains__("max_var") else 1
        self.eta = model_params.eta if model_params.__contains__("eta") else 1
        self.skip_sample = model_params.skip_sample
        self.sample_type = model_params.sample_type
        self.sample_step = model_params.sample_step
        self.steps = None
        self.register_schedule()

        self.loss_type = model_params.loss_type
        self.objective = model_params.objective

        self.image_size = model_params.UNetParams.image_size
        self.channels = model_params.UNetParams.in_channels
        self.condition_key = model_params.UNetParams.condition_key

        self.denoise_fn = UNetModel(**vars(model_params.UNetParams))

    # ------------------------------------------------------------------------------------------------------
    def register_schedule(self):
        """Schedule buffers + sampling step table (BrownianBridgeModel.py:42-79).  Host-side float64 -> fp32 buffers
        that are part of the ``state_dict``; ``self.steps`` stays a CPU tensor attribute as in the reference."""
        tables, self.steps = bridge_schedule(self.num_timesteps, self.mt_type, self.max_var, self.skip_sample,
                                             self.sample_type, self.sample_step)
        for name, values in tables.items():
            self.register_buffer(name, torch.tensor(values, dtype=torch.float32))
        self._steps_list = None

    def _steps_host(self):
        """``steps`` as a Python list (it is a CPU tensor attribute in the reference too: no device sync)."""
        if self._steps_list is None or len(self._steps_list) != len(self.steps):
            self._steps_list = [int(s) for s in self.steps]
        return self._steps_list

    def apply(self, weight_init):
        self.denoise_fn.apply(weight_init)
        return self

    def get_parameters(self):
        return self.denoise_fn.parameters()

    # ------------------------------------------------------------------------------------------------------
    def forward(self, x, y, context=None):
        """BrownianBridgeModel.py:88-96."""
        if self.condition_key == "nocond":
            context = None
        else:
            context = y if context is None else context
        b, c, h, w, device, img_size, = *x.shape, x.device, self.image_size
        assert h == img_size and w == img_size, f'height and width of image must be {img_size}'
        t = torch.randint(0, self.num_timesteps, (b,), device=device).long()
        return self.p_losses(x, y, context, t)

    def p_losses(self, x0, y, context, t, noise=None, seeds=None, ordinals=None):
        """BrownianBridgeModel.py:98-126.  ``seeds`` (one per sample, e.g. base + dataset index; ``ordinals`` default 0, meant for
        the caller's global step): the noise is generated inside the q_sample kernel, a function of (seed, ordinal) that does not
        depend on how the samples are sharded over ranks."""
        if self.loss_type not in _LOSSES:
            raise NotImplementedError()
        if seeds is None:
            noise = torch.randn_like(x0) if noise is None else noise
        x_t, objective = self.q_sample(x0, y, t, noise, seeds=seeds, ordinals=ordinals)
        return self._denoise_and_loss(x_t, objective, y, context, t)

    def _denoise_and_loss(self, x_t, objective, y, context, t):
        """BrownianBridgeModel.py:107-126: everything of p_losses after q_sample."""
        objective_recon = self.denoise_fn(x_t, timesteps=t, context=context)
        if objective_recon.requires_grad:
            from .autograd import bb_loss      # differentiable HIP loss (training path)
            recloss = bb_loss(objective, objective_recon, self.loss_type)
        else:
            recloss = self._loss(objective, objective_recon)
        meter = self._loss_meters[0 if self.training else 1]
        if meter is not None:                  # the loss by timestep (bbdm_amd/loss_meter.py): two launches, no read-back
            meter.add(objective, objective_recon.detach(), t, loss_type=self.loss_type)
        x0_recon = self.predict_x0_from_objective(x_t, y, t, objective_recon.detach())
        log_dict = {"loss": recloss, "x0_recon": x0_recon}
        return recloss, log_dict

    # ---- loss meters (bbdm_amd/loss_meter.py) -----------------------------------------------------------
    _loss_meters = (None, None)

    def attach_loss_meter(self, train=None, val=None):
        """From here on every loss evaluation (``forward``, ``p_losses``, ``p_losses_cached``) also adds its per-image losses and their
        ``t`` to a :class:`bbdm_amd.LossMeter`: ``train`` while ``self.training``, ``val`` otherwise; either may be None.  The loss,
        its gradient and the keys of ``log_dict`` are what they are without a meter."""
        for m in (train, val):
            if m is not None and m.num_timesteps != self.num_timesteps:
                raise ValueError(f"the meter buckets {m.num_timesteps} timesteps, the model has {self.num_timesteps}")
        self._loss_meters = (train, val)

    def detach_loss_meter(self):
        self._loss_meters = (None, None)

    def _loss(self, a, b):
        _need_gpu(a, b)
        a, b = _f32c(a), _f32c(b)
        partial_ = torch.zeros(4, dtype=torch.float64, device=a.device)       # one exact limb cell (csrc/stats_acc.h)
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        _launch(a, "bbdm_bb_loss_f32", a.data_ptr(), b.data_ptr(), partial_.data_ptr(), out.data_ptr(), a.numel(),
                  _LOSSES[self.loss_type])
        return out[0]

    def _table_index(self, t):
        """``t`` as the contiguous int64 index the kernels read ``m_t`` / ``variance_t`` with, clamped to ``[0, num_timesteps)`` on the
        device (one small launch, no sync).  The kernels take the tables as bare pointers: an out-of-range ``t`` -- where the reference
        raises from its gather -- read whatever lay beside the tables, so a result could depend on the heap's layout.  In-range ``t``
        is unchanged; the UNet's timestep embedding and an attached loss meter (which rejects it) still see the caller's ``t``."""
        return t.to(torch.int64).clamp(0, self.num_timesteps - 1).contiguous()

    def q_sample(self, x0, y, t, noise=None, seeds=None, ordinals=None):
        """BrownianBridgeModel.py:128-146 -> (x_t, objective).  With ``seeds``: noise = philox_normal(shape, seeds, ordinals,
        domain=1), generated in the kernel's registers."""
        if self.objective not in _OBJECTIVES:
            raise NotImplementedError()
        if seeds is not None:
            if noise is not None:
                raise ValueError("q_sample: pass noise or seeds, not both")
            return self._q_sample_seeded(x0, y, t, seeds, 0 if ordinals is None else ordinals)
        if ordinals is not None:
            raise ValueError("q_sample: ordinals without seeds")
        noise = torch.randn_like(x0) if noise is None else noise
        _need_gpu(x0, y, noise, t)
        x0c, yc, nc = _f32c(x0), _f32c(y), _f32c(noise)
        tc = self._table_index(t)
        x_t, target = torch.empty_like(x0c), torch.empty_like(x0c)
        _launch(x0c, "bbdm_bb_q_sample_f32", x0c.data_ptr(), yc.data_ptr(), nc.data_ptr(), tc.data_ptr(),
                  self.m_t.data_ptr(), self.variance_t.data_ptr(), x_t.data_ptr(), target.data_ptr(),
                  x0c.shape[0], x0c[0].numel(), _OBJECTIVES[self.objective])
        return x_t, target

    def _q_sample_seeded(self, x0, y, t, seeds, ordinals):
        _need_gpu(x0, y, t)
        x0c, yc = _f32c(x0), _f32c(y)
        tc = self._table_index(t)
        n = x0c.shape[0]
        sd = _i64_per_image(seeds, n, x0c.device, "seeds")
        od = _i64_per_image(ordinals, n, x0c.device, "ordinals")
        x_t, target = torch.empty_like(x0c), torch.empty_like(x0c)
        _launch(x0c, "bbdm_bb_q_sample_philox_f32", x0c.data_ptr(), yc.data_ptr(), sd.data_ptr(), od.data_ptr(), tc.data_ptr(),
                  self.m_t.data_ptr(), self.variance_t.data_ptr(), x_t.data_ptr(), target.data_ptr(), n, x0c[0].numel(),
                  _OBJECTIVES[self.objective])
        return x_t, target

    def predict_x0_from_objective(self, x_t, y, t, objective_recon):
        """BrownianBridgeModel.py:148-160."""
        if self.objective not in _OBJECTIVES:
            raise NotImplementedError
        _need_gpu(x_t, y, objective_recon, t)
        a, b, p = _f32c(x_t), _f32c(y), _f32c(objective_recon)
        tc = self._table_index(t)
        out = torch.empty_like(a)
        _launch(a, "bbdm_bb_predict_x0_f32", a.data_ptr(), b.data_ptr(), p.data_ptr(), tc.data_ptr(),
                  self.m_t.data_ptr(), self.variance_t.data_ptr(), out.data_ptr(), a.shape[0], a[0].numel(),
                  _OBJECTIVES[self.objective])
        return out

    @torch.no_grad()
    def q_sample_loop(self, x0, y):
        """BrownianBridgeModel.py:162-169."""
        imgs = [x0]
        for i in tqdm(range(self.num_timesteps), desc='q sampling loop', total=self.num_timesteps):
            t = torch.full((y.shape[0],), i, device=x0.device, dtype=torch.long)
            img, _ = self.q_sample(x0, y, t)
            imgs.append(img)
        return imgs

    # ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def p_sample(self, x_t, y, context, i, clip_denoised=False, seeds=None):
        """BrownianBridgeModel.py:171-201: one UNet call + ONE fused update kernel -> (x_{t-1}, x0_recon).  ``seeds`` (one per
        image): the step's noise is philox_normal(shape, seeds, i), generated inside the update kernel."""
        if self.objective not in _OBJECTIVES:
            raise NotImplementedError
        _need_gpu(x_t, y)
        steps = self._steps_host()
        step = steps[i]
        nxt = 0 if step == 0 else steps[i + 1]
        if not (0 <= step < self.num_timesteps and 0 <= nxt < self.num_timesteps):
            # the reference gathers m_t[t] and fails there (sample_type 'cosine' starts at t = num_timesteps:
            # BrownianBridgeModel.py:74-77); the kernels read the tables unchecked, so the check lives here
            raise IndexError(f"timestep {max(step, nxt)} is out of range for the {self.num_timesteps}-entry schedule")
        x_t, y = _f32c(x_t), _f32c(y)
        fn = self.denoise_fn
        plan = None
        if isinstance(fn, UNetModel):
            # the prediction is consumed by the fused kernel below at once (no per-step copy of it); the timestep is a host integer
            # (one fill of the plan's buffer instead of torch.full + copy); the plan skips the copies of inputs it already holds
            objective_recon, plan = fn.infer_step(x_t, step, context)
        else:
            t = torch.full((x_t.shape[0],), step, device=x_t.device, dtype=torch.long)
            objective_recon = fn(x_t, timesteps=t, context=context)
        is_last = step == 0
        x_next, x0_recon = torch.empty_like(x_t), torch.empty_like(x_t)
        # the loop feeds x_next back as the next x_t (BrownianBridgeModel.py:218-220): the step writes it into the plan's input buffer too
        alias = None if (plan is None or is_last) else plan.x_in
        if seeds is not None:
            n = x_t.shape[0]
            sd = _i64_per_image(seeds, n, x_t.device, "seeds")
            # step, next step, flag (0 a step with noise, 1 the last one) and ordinal of every image: one upload
            idx = torch.tensor([[step] * n, [nxt] * n, [1 if is_last else 0] * n, [i] * n], dtype=torch.int64).to(x_t.device)
            _launch(x_t, "bbdm_bb_p_sample_step_philox_f32", x_t.data_ptr(), y.data_ptr(), objective_recon.data_ptr(),
                      sd.data_ptr(), idx[3].data_ptr(), self.m_t.data_ptr(), self.variance_t.data_ptr(), idx[0].data_ptr(),
                      idx[1].data_ptr(), idx[2].data_ptr(), float(self.eta), 1 if clip_denoised else 0,
                      _OBJECTIVES[self.objective], x_next.data_ptr(), x0_recon.data_ptr(),
                      None if alias is None else alias.data_ptr(), n, x_t[0].numel())
            if alias is not None:
                plan.holds_input(x_next)
            if is_last:
                return x0_recon, x0_recon
            return x_next, x0_recon
        noise = None if is_last else torch.randn_like(x_t)
        _launch(x_t, "bbdm_bb_p_sample_step_f32", x_t.data_ptr(), y.data_ptr(), objective_recon.data_ptr(),
                  None if noise is None else noise.data_ptr(), self.m_t.data_ptr(), self.variance_t.data_ptr(),
                  step, 0 if is_last else steps[i + 1], 1 if is_last else 0, float(self.eta),
                  1 if clip_denoised else 0, _OBJECTIVES[self.objective], x_next.data_ptr(), x0_recon.data_ptr(),
                  None if alias is None else alias.data_ptr(), x_t.shape[0], x_t[0].numel())
        if alias is not None:
            plan.holds_input(x_next)
        if is_last:
            return x0_recon, x0_recon
        return x_next, x0_recon

    @torch.no_grad()
    def p_sample_loop(self, y, context=None, clip_denoised=True, sample_mid_step=False, seeds=None):
        """BrownianBridgeModel.py:203-221.  ``seeds`` (int64 tensor or sequence, one per image): seed-addressed noise, step i of
        image n drawing philox_normal(shape, seeds[n], i)."""
        if self.condition_key == "nocond":
            context = None
        else:
            context = y if context is None else context
        if seeds is not None:
            seeds = _i64_per_image(seeds, y.shape[0], y.device, "seeds")         # uploaded once for the whole loop

        if sample_mid_step:
            imgs, one_step_imgs = [y], []
            for i in tqdm(range(len(self.steps)), desc=f'sampling loop time step', total=len(self.steps)):
                img, x0_recon = self.p_sample(x_t=imgs[-1], y=y, context=context, i=i, clip_denoised=clip_denoised, seeds=seeds)
                imgs.append(img)
                one_step_imgs.append(x0_recon)
            return imgs, one_step_imgs
        else:
            img = y
            for i in tqdm(range(len(self.steps)), desc=f'sampling loop time step', total=len(self.steps)):
                img, _ = self.p_sample(x_t=img, y=y, context=context, i=i, clip_denoised=clip_denoised, seeds=seeds)
            return img

    @torch.no_grad()
    def sample(self, y, context=None, clip_denoised=True, sample_mid_step=False, seeds=None):
        """BrownianBridgeModel.py:223-225."""
        return self.p_sample_loop(y, context, clip_denoised, sample_mid_step, seeds=seeds)


def disabled_train(self, mode=True):
    """Bound over ``vqgan.train`` so later ``.train()`` calls cannot un-freeze it (LatentBrownianBridgeModel.py:13-16)."""
    return self


class LatentBrownianBridgeModel(BrownianBridgeModel):
    """LatentBrownianBridgeModel.py:19-147: the same bridge run in the latent space of a frozen VQGAN.

    Only the wrapper API lives here (constructor, ``forward``, ``encode``/``decode``, ``sample``, the externally
    assigned ``ori_latent_mean/std`` and ``cond_latent_mean/std`` attributes -- BBDMRunner.py:41-44).  The first stage
    is any module exposing ``encoder / quant_conv / quantize / decode``: by default ``bbdm_amd.first_stage_hip.VQModel``
    built from ``model_config.VQGAN.params`` (encode / decode on the HIP kernels for GPU tensors; loads the reference's VQGAN
    checkpoints), or whatever is passed as ``vqgan=`` (e.g. the checkout's own ``model.VQGAN.vqgan.VQModel``).  The first stage
    is the ONE place with a PyTorch branch: a foreign ``vqgan`` without ``encode_latent`` / ``decode_latent``, or CPU tensors, go
    through the module's own PyTorch ``encoder`` / ``quantize`` / ``decode`` (north_star leaves the VQGAN on PyTorch-ROCm); the UNet
    and the bridge have none.
    """

    def __init__(self, model_config, vqgan: nn.Module = None):
        super().__init__(model_config)
        if vqgan is None:
            # state_dict-compatible with the reference's VQModel; encode / decode run on the HIP kernels
            from .first_stage_hip import VQModel
            vqgan = VQModel(**vars(model_config.VQGAN.params))
        self.vqgan = vqgan.eval()
        self.vqgan.train = disabled_train
        self.vqgan.requires_grad_(False)
        print(f"load vqgan from {getattr(model_config.VQGAN.params, 'ckpt_path', None)}")

        key = self.condition_key
        if key == 'nocond':
            self.cond_stage_model = None
        elif key == 'first_stage':
            self.cond_stage_model = self.vqgan
        elif key == 'SpatialRescaler':
            from .cond_stage import SpatialRescaler          # same constructor / state_dict as the reference's class
            self.cond_stage_model = SpatialRescaler(**vars(model_config.CondStageParams))
        else:
            raise NotImplementedError

    def get_ema_net(self):
        return self

    def get_parameters(self):
        unet = self.denoise_fn.parameters()
        if self.condition_key != 'SpatialRescaler':
            print("get parameters to optimize: UNet")
            return unet
        print("get parameters to optimize: SpatialRescaler, UNet")
        return itertools.chain(unet, self.cond_stage_model.parameters())

    def apply(self, weights_init):
        BrownianBridgeModel.apply(self, weights_init)
        if self.cond_stage_model is not None:
            self.cond_stage_model.apply(weights_init)
        return self

    # ---- latent cache (bbdm_amd/latent_cache.py) -------------------------------------------------------
    _latent_cache = None

    def attach_latent_cache(self, cache):
        """From here on ``forward`` accepts int64 index tensors [N] in place of the two image batches and reads the latents from
        ``cache`` (a :class:`bbdm_amd.latent_cache.LatentCache`) instead of running the frozen encoder.  Image inputs keep their
        path.  The cache holds no context, so the model must be ``nocond`` (LatentCache.build refuses the others too)."""
        if self.cond_stage_model is not None:
            raise ValueError(f"a latent cache cannot serve condition_key {self.condition_key!r}: its context is computed from the pixels")
        if tuple(cache.ori.shape) != tuple(cache.cond.shape) or cache.ori.dim() != 4:
            raise ValueError(f"latent cache tensors must be two equal [M, C, h, w], got {tuple(cache.ori.shape)} / {tuple(cache.cond.shape)}")
        _need_gpu(cache.ori, cache.cond)
        self._latent_cache = cache

    def detach_latent_cache(self):
        self._latent_cache = None

    def _cache_indices(self, idx, M, device, what):
        """int64 [N] on the device.  Indices that arrive on the CPU are range-checked here; indices already on the device are not read
        back (no sync): the kernel answers an out-of-range one with NaN rows for that image -- see ``skip_nonfinite`` in
        bbdm_amd/optim.py, which then skips the step."""
        if not idx.is_cuda and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= M):
            raise IndexError(f"{what}: index out of range for a latent cache of {M} rows")
        return idx.to(device=device, dtype=torch.int64).contiguous()

    def _forward_cached(self, idx_ori, idx_cond):
        if idx_ori.dim() != 1 or tuple(idx_cond.shape) != tuple(idx_ori.shape) or torch.is_floating_point(idx_cond):
            raise ValueError(f"latent-cache indices must be two integer tensors [N], got {tuple(idx_ori.shape)} {idx_ori.dtype} / "
                             f"{tuple(idx_cond.shape)} {idx_cond.dtype}")
        cache = self._latent_cache
        if cache is None:
            raise RuntimeError("integer inputs are rows of a latent cache, and none is attached (attach_latent_cache)")
        h, w, img_size = cache.ori.shape[2], cache.ori.shape[3], self.image_size
        assert h == img_size and w == img_size, f'height and width of image must be {img_size}'
        # the same call as BrownianBridgeModel.forward: the generator advances identically on both paths
        t = torch.randint(0, self.num_timesteps, (idx_ori.shape[0],), device=cache.ori.device).long()
        return self.p_losses_cached(idx_ori, idx_cond, t)

    def p_losses_cached(self, idx_ori, idx_cond, t, noise=None, seeds=None, ordinals=None):
        """``p_losses`` on rows of the attached cache: one gather + normalise + q_sample kernel, then the UNet, the loss and x0_recon
        as in ``p_losses``.  ``noise`` / ``seeds`` / ``ordinals`` as there; no encoder launch happens here."""
        if self.loss_type not in _LOSSES:
            raise NotImplementedError()
        if self.objective not in _OBJECTIVES:
            raise NotImplementedError()
        cache = self._latent_cache
        if cache is None:
            raise RuntimeError("no latent cache attached (attach_latent_cache)")
        ori, cond = cache.ori, cache.cond
        M, C, hw, dev = ori.shape[0], ori.shape[1], ori.shape[2] * ori.shape[3], ori.device
        io = self._cache_indices(idx_ori, M, dev, "idx_ori")
        ic = self._cache_indices(idx_cond, M, dev, "idx_cond")
        n = io.shape[0]
        if ic.shape[0] != n:
            raise ValueError(f"idx_cond: {ic.shape[0]} indices for {n} images")
        if seeds is not None and noise is not None:
            raise ValueError("p_losses_cached: pass noise or seeds, not both")
        if seeds is None and ordinals is not None:
            raise ValueError("p_losses_cached: ordinals without seeds")
        stats = [None] * 4
        if self.model_config.normalize_latent:              # read at call time, like encode()
            stats = [_f32c(v.to(dev).reshape(-1)) for v in self._latent_stats(False) + self._latent_stats(True)]
            if any(v.numel() != C for v in stats):
                raise ValueError(f"latent mean / std must have {C} channels")
        tc = t.to(torch.int64).contiguous()
        _need_gpu(ori, cond, tc)
        x_t, target, y = (torch.empty((n,) + tuple(ori.shape[1:]), dtype=torch.float32, device=dev) for _ in range(3))
        head = (ori.data_ptr(), cond.data_ptr(), M, io.data_ptr(), ic.data_ptr(), *(None if v is None else v.data_ptr() for v in stats), hw)
        tq = self._table_index(tc)
        tail = (tq.data_ptr(), self.m_t.data_ptr(), self.variance_t.data_ptr(), x_t.data_ptr(), target.data_ptr(), y.data_ptr(),
                n, C * hw, _OBJECTIVES[self.objective])
        if seeds is not None:
            sd = _i64_per_image(seeds, n, dev, "seeds")
            od = _i64_per_image(0 if ordinals is None else ordinals, n, dev, "ordinals")
            _launch(ori, "bbdm_bb_q_sample_cached_philox_f32", *head, sd.data_ptr(), od.data_ptr(), *tail)
        else:
            noise = _f32c(torch.randn(x_t.shape, dtype=torch.float32, device=dev) if noise is None else noise)
            _need_gpu(noise)
            if tuple(noise.shape) != tuple(x_t.shape):
                raise ValueError(f"noise must be {tuple(x_t.shape)}, got {tuple(noise.shape)}")
            _launch(ori, "bbdm_bb_q_sample_cached_f32", *head, noise.data_ptr(), *tail)
        return self._denoise_and_loss(x_t, target, y, None, tc)

    def forward(self, x, x_cond, context=None):
        if not torch.is_floating_point(x):                  # rows of the attached latent cache instead of images
            return self._forward_cached(x, x_cond)
        # both images go through the frozen encoder without a graph; only the UNet (+ rescaler) is trained
        with torch.no_grad():
            latents = [self.encode(img, cond=flag).detach() for img, flag in ((x, False), (x_cond, True))]
        return BrownianBridgeModel.forward(self, latents[0], latents[1], self.get_cond_stage_context(x_cond))

    def get_cond_stage_context(self, x_cond):
        if self.cond_stage_model is None:
            return None
        context = self.cond_stage_model(x_cond)
        return context.detach() if self.condition_key == 'first_stage' else context

    def _latent_stats(self, cond):
        if cond:
            return self.cond_latent_mean, self.cond_latent_std
        return self.ori_latent_mean, self.ori_latent_std

    def _use_norm(self, normalize):
        return self.model_config.normalize_latent if normalize is None else normalize

    @torch.no_grad()
    def encode(self, x, cond=True, normalize=None):
        if hasattr(self.vqgan, "encode_latent") and x.is_cuda:      # bbdm_amd.first_stage_hip: the whole encoder on HIP
            z = self.vqgan.encode_latent(x, quant_conv=not self.model_config.latent_before_quant_conv)
        else:
            z = self.vqgan.encoder(x)
            if not self.model_config.latent_before_quant_conv:
                z = self.vqgan.quant_conv(z)
        if self._use_norm(normalize):
            mean, std = self._latent_stats(cond)
            z = (z - mean) / std
        return z

    @torch.no_grad()
    def decode(self, x_latent, cond=True, normalize=None):
        z = x_latent
        if self._use_norm(normalize):
            mean, std = self._latent_stats(cond)
            z = z * std + mean
        if hasattr(self.vqgan, "decode_latent") and z.is_cuda:      # quantize + post_quant_conv + decoder on HIP
            return self.vqgan.decode_latent(z, quant_conv_first=self.model_config.latent_before_quant_conv)
        if self.model_config.latent_before_quant_conv:
            z = self.vqgan.quant_conv(z)
        z_q, _, _ = self.vqgan.quantize(z)
        return self.vqgan.decode(z_q)

    @torch.no_grad()
    def sample(self, x_cond, clip_denoised=False, sample_mid_step=False, seeds=None):
        result = self.p_sample_loop(y=self.encode(x_cond, cond=True), context=self.get_cond_stage_context(x_cond),
                                    clip_denoised=clip_denoised, sample_mid_step=sample_mid_step, seeds=seeds)
        if not sample_mid_step:
            return self.decode(result, cond=False)

        def decode_all(latents, desc):
            return [self.decode(z.detach(), cond=False).to('cpu')
                    for z in tqdm(latents, initial=0, desc=desc, dynamic_ncols=True, smoothing=0.01)]

        trajectory, one_step = result
        return (decode_all(trajectory, "save output sample mid steps"),
                decode_all(one_step, "save one step sample mid steps"))

    @torch.no_grad()
    def sample_vqgan(self, x):
        return self.vqgan(x)[0]
