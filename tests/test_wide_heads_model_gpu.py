"""UNets with 128-channel attention heads (GPU): a tiny UNet whose attention layers are 128 wide -- AttentionBlock in the legacy and the
new head order, and a SpatialTransformer with a context -- against the oracle (sampling forward at the model tests' bar; loss and every
parameter gradient against autograd), a bitwise reproducible training step, and the C2 pixel UNet with `num_head_channels: -1`
(8 heads of 128 at 1024 channels, T = 4096), one p_sample step at 256 x 256."""
import pytest
import torch

import bbdm_oracle as O
import test_fullsize_parity_gpu as FS
from fixtures import parity_err

pytestmark = pytest.mark.gpu
STEP_TOL = 1e-4          # test_model_gpu.py
GRAD_TOL = 1e-3          # test_training_gpu.py: per-parameter max|g - g_ref| / max|g_ref|

TINY = dict(image_size=16, in_channels=6, model_channels=64, out_channels=3, num_res_blocks=1, attention_resolutions=(1, 2),
            channel_mult=(1, 2), conv_resample=True, dims=2, num_heads=8, num_head_channels=128, use_scale_shift_norm=True,
            resblock_updown=True, use_spatial_transformer=False, context_dim=None, condition_key="SpatialRescaler")
VARIANTS = {
    # (ds 1: 128 channels -> one head of 128; ds 2: 256 channels -> two heads of 128)
    "attention_legacy": dict(TINY, model_channels=128, num_head_channels=128),
    "attention_new_order": dict(TINY, model_channels=128, num_head_channels=128, use_new_attention_order=True),
    # SpatialTransformer, the same head widths; its cross-attention reads the 3-channel context (the condition image)
    "spatial_transformer": dict(TINY, model_channels=128, num_head_channels=128, use_spatial_transformer=True, context_dim=3),
}
BB = dict(FS.BB, sample_step=10)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _widths(m):
    from bbdm_amd import unet
    w = {mod.channels // mod.num_heads for mod in m.modules() if isinstance(mod, unet.AttentionBlock)}
    return w | {mod.d_head for mod in m.modules() if isinstance(mod, unet.SpatialTransformer)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tiny_unet_forward_matches_oracle(dev, variant):
    up = VARIANTS[variant]
    m, sd = FS._model(up, BB, 128, dev)
    m.eval()
    assert 128 in _widths(m.denoise_fn)
    g = torch.Generator().manual_seed(5)
    N = 2
    x = torch.randn(N, 3, 16, 16, generator=g)
    y = torch.randn(N, 3, 16, 16, generator=g).clamp(-1, 1)
    t = torch.tensor([3, 800])
    with torch.no_grad():       # (condition "SpatialRescaler": the UNet input is x | context, openaimodel.py:721-759)
        out = m.denoise_fn(x.to(dev), timesteps=t.to(dev), context=y.to(dev))
        torch.cuda.synchronize()
        ref = O.unet_forward(sd, O.UNetSpec(**up), x, t, y)
    e = parity_err(out.cpu(), ref)
    print(f"tiny UNet ({variant}): forward rel err {e:.2e}")
    assert e < STEP_TOL
    eps = torch.randn(N, 3, 16, 16, generator=g)
    ora = O.OracleBBDM({"denoise_fn." + k: v for k, v in sd.items()}, O.UNetSpec(**up), **BB)
    with torch.no_grad():
        a_ref, b_ref = ora.p_sample(x, y, y, 4, clip_denoised=False, noise=eps)
    a, b = FS._p_sample(m, x, y, y, 4, eps, dev)
    assert parity_err(a, a_ref) < STEP_TOL and parity_err(b, b_ref) < STEP_TOL


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tiny_unet_loss_and_all_gradients(dev, variant):
    up = VARIANTS[variant]
    bb = dict(BB, loss_type="l2")          # (l1's sign pattern is discontinuous: see test_fullsize_parity_gpu.py's C4 test)
    m, sd = FS._model(up, bb, 129, dev)
    m.train()
    g = torch.Generator().manual_seed(9)
    N = 2
    x0 = torch.randn(N, 3, 16, 16, generator=g)
    y = torch.randn(N, 3, 16, 16, generator=g)
    t = torch.tensor([612, 37])
    nz = torch.randn(N, 3, 16, 16, generator=g)
    sd_o = {"denoise_fn." + k: v.clone().requires_grad_() for k, v in sd.items()}
    lo, _ = O.OracleBBDM(sd_o, O.UNetSpec(**up), **bb).p_losses(x0, y, y, t, nz)
    lo.backward()
    l_ref, g_ref = float(lo.detach()), {k[len("denoise_fn."):]: v.grad for k, v in sd_o.items()}
    grads = []
    for rep in range(2):
        m.zero_grad(set_to_none=True)
        loss, _ = m.p_losses(x0.to(dev), y.to(dev), y.to(dev), t.to(dev), nz.to(dev))
        loss.backward()
        torch.cuda.synchronize()
        grads.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.denoise_fn.named_parameters()}))
    lv = float(grads[0][0])
    assert abs(lv - l_ref) < 1e-5 * max(1.0, abs(l_ref))
    gmax = max(float(v.abs().max()) for v in g_ref.values())
    rows = sorted(((float((grads[0][1][k].cpu() - g_ref[k]).abs().max()) / max(float(g_ref[k].abs().max()), 1e-3 * gmax), k)
                   for k in grads[0][1]), reverse=True)
    print(f"tiny UNet ({variant}) gradients: loss {lv:.6f} (oracle {l_ref:.6f}); worst: " + "; ".join(f"{k} {e:.2e}" for e, k in rows[:3]))
    assert rows[0][0] < GRAD_TOL, rows[0]
    # a training step is bitwise reproducible
    assert torch.equal(grads[0][0], grads[1][0])
    assert all(torch.equal(grads[0][1][k], grads[1][1][k]) for k in grads[0][1])


def test_c2_pixel_unet_with_8_heads_of_128(dev):
    """The C2 template with `num_head_channels: -1`: the reference then takes `num_heads: 8` (openaimodel.py:546-553), 1024 / 8 = 128
    channels per head on the 1024-channel layers, incl. the T = 4096 layer.  One p_sample step at 256 x 256, batch 1."""
    up = dict(FS.UNET_PIXEL, image_size=256, num_head_channels=-1)
    m, sd = FS._model(up, dict(FS.BB, skip_sample=False), 778, dev)
    m.eval()
    assert 128 in _widths(m.denoise_fn)
    g = torch.Generator().manual_seed(4321)
    S = 256
    y = torch.randn(1, 3, S, S, generator=g).clamp(-1, 1)
    x_t = torch.randn(1, 3, S, S, generator=g).clamp(-1, 1)
    eps = torch.randn(1, 3, S, S, generator=g)
    ora = O.OracleBBDM({"denoise_fn." + k: v for k, v in sd.items()}, O.UNetSpec(**up), **dict(FS.BB, skip_sample=False))
    i = 431
    with torch.no_grad():
        a_ref, b_ref = ora.p_sample(x_t, y, y, i, clip_denoised=False, noise=eps)
    a, b = FS._p_sample(m, x_t, y, y, i, eps, dev)
    plan = next(iter(m.denoise_fn._plans.values()))
    # the T = 4096 layer: the pre-split pair on the fp16-pair planes, as the 16 x 64 form of the layer runs
    geo = {(str(getattr(n, "entry", n)), tuple(args[6:9])) for n, args in plan.ops if str(n) == "bbdm_attention_f32"}
    assert ("bbdm_attention_planes_h2_f32", (4096, 8, 128)) in geo, geo
    ea, eb = parity_err(a, a_ref), parity_err(b, b_ref)
    print(f"C2 256x256 step, 8 heads x 128, batch 1: rel err x_tminus {ea:.2e}  x0_recon {eb:.2e}")
    assert ea < 1e-3 and eb < 1e-3
    m.denoise_fn._plans = {}
    torch.cuda.empty_cache()
