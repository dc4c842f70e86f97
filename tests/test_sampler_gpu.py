"""BridgeSampler (bbdm_amd/sampler.py) on the GPU: the per-image bridge kernel against the scalar one, lockstep runs against
``p_sample_loop`` / ``LatentBrownianBridgeModel.sample`` bit for bit, and mixed progress against the oracle's loops."""
import argparse
import contextlib

import pytest
import torch

import sampler_cases as S
import test_fullsize_parity_gpu as FS
from fixtures import load_case, oracle_model, parity_err

pytestmark = pytest.mark.gpu

TINY = dict(image_size=16, in_channels=6, model_channels=64, out_channels=3, num_res_blocks=1, attention_resolutions=(2,),
            channel_mult=(1, 2), conv_resample=True, dims=2, num_heads=2, num_head_channels=32, use_scale_shift_norm=True,
            resblock_updown=True, use_spatial_transformer=False, context_dim=None, condition_key="SpatialRescaler")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@contextlib.contextmanager
def stacked_randn_like(gens, dev):
    """torch.randn_like patched to return the stacked per-request draws of the sampler's noise contract."""
    orig = torch.randn_like
    torch.randn_like = lambda t, **k: torch.stack([torch.randn(tuple(t.shape[1:]), generator=g, device=dev) for g in gens])
    try:
        yield
    finally:
        torch.randn_like = orig


def _gens(seeds, dev):
    out = []
    for s in seeds:
        g = torch.Generator(device=dev)
        g.manual_seed(s)
        out.append(g)
    return out


def test_batched_bridge_step_is_bit_equal_to_the_scalar_step(dev):
    S.kernel_equivalence(dev)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("key", ["SpatialRescaler", "nocond"])
def test_lockstep_group_equals_p_sample_loop(dev, key, clip):
    up = dict(TINY, condition_key=key, in_channels=6 if key != "nocond" else 3)
    m, _ = FS._model(up, dict(FS.BB, sample_step=10), 5150, dev)
    m.eval()
    from bbdm_amd import BridgeSampler
    g = torch.Generator().manual_seed(3)
    conds = torch.randn(4, 3, 16, 16, generator=g).clamp(-1, 1).to(dev)
    seeds = [71, 72, 73, 74]
    s = BridgeSampler(m, 4, clip_denoised=clip)
    s.submit([(k, conds[k], gen) for k, gen in enumerate(_gens(seeds, dev))])
    got = dict(s)
    assert sorted(got) == [0, 1, 2, 3]
    with stacked_randn_like(_gens(seeds, dev), dev):
        ref = m.p_sample_loop(conds, None, clip_denoised=clip)
    torch.cuda.synchronize()
    out = torch.stack([got[k] for k in range(4)])
    assert torch.equal(out, ref), float((out - ref).abs().max())


def test_mixed_progress_follows_the_oracle_in_any_slot(dev):
    """Default plan (fp16-pair planes on), 7 requests, width 4, sample_step 10: every request within 5e-3 of its own oracle loop; request 3
    (slot 3 there) again in slot 0 of a second sampler with other batch-mates, within 5e-3 both times."""
    from bbdm_amd import BridgeSampler
    m, s, conds, seeds, ora = S.mixed_progress(dev, 4, 7, 10, clip=True)
    assert m.denoise_fn.gemm_h2
    k = 3
    g = torch.Generator().manual_seed(99)
    mates = torch.randn(5, 3, 16, 16, generator=g).clamp(-1, 1).to(dev)
    s2 = BridgeSampler(m, 4, clip_denoised=True)
    reqs = [(k, conds[k], _gens([seeds[k]], dev)[0])] + [(100 + j, mates[j], _gens([500 + j], dev)[0]) for j in range(5)]
    s2.submit(reqs)
    s2.step()
    assert s2._slots[0][0].key == k
    got = dict(s2)
    ref = S.oracle_loop(ora, conds[k], True, seeds[k], dev)
    err = parity_err(got[k].cpu(), ref)
    print(f"request {k} in slot 0 with other batch-mates: {err:.2e}")
    assert err < S.LOOP_TOL


def _latent_model(dev):
    import bbdm_amd
    rec = load_case("tiny_nocond")
    dd = dict(double_z=False, z_channels=8, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2, 2),
              num_res_blocks=1, attn_resolutions=[], dropout=0.0)
    cfg = S._ns({"BB": {"params": dict(rec["bb_params"], UNetParams=rec["unet_params"])},
                 "VQGAN": {"params": {"ckpt_path": None, "embed_dim": 8, "n_embed": 128, "ddconfig": dd,
                                      "lossconfig": {"target": "torch.nn.Identity"}}},
                 "normalize_latent": False, "latent_before_quant_conv": False})
    torch.manual_seed(4)
    m = bbdm_amd.LatentBrownianBridgeModel(cfg).to(dev)
    m.denoise_fn.load_state_dict({k[len("denoise_fn."):]: v for k, v in rec["state_dict"].items() if k.startswith("denoise_fn.")})
    return m.eval(), oracle_model(rec)


def test_latent_sampler_lockstep_and_mixed_progress(dev):
    from bbdm_amd import BridgeSampler
    m, ora = _latent_model(dev)
    g = torch.Generator().manual_seed(8)
    conds = torch.randn(6, 3, 32, 32, generator=g).clamp(-1, 1).to(dev)
    seeds = [300 + k for k in range(6)]
    # lockstep: one group of 4 == model.sample on the same 4 conditions with the same noise
    s = BridgeSampler(m, 4)
    s.submit([(k, conds[k], gen) for k, gen in enumerate(_gens(seeds[:4], dev))])
    got = dict(s)
    with stacked_randn_like(_gens(seeds[:4], dev), dev):
        ref = m.sample(conds[:4], clip_denoised=False)
    torch.cuda.synchronize()
    out = torch.stack([got[k] for k in range(4)])
    assert out.shape == (4, 3, 32, 32) and torch.equal(out, ref), float((out - ref).abs().max())
    # mixed progress: 6 requests, width 4, arriving in two groups two steps apart; each within 5e-3 of the oracle's latent loop from the
    # same y, decoded by the same first stage
    s = BridgeSampler(m, 4)
    gens = _gens(seeds, dev)
    s.submit([(k, conds[k], gens[k]) for k in range(3)])
    got = {}
    for _ in range(2):
        got.update(s.step())
    s.submit([(k, conds[k], gens[k]) for k in range(3, 6)])
    got.update(dict(s))
    assert sorted(got) == list(range(6))
    for k in range(6):
        y = m.encode(conds[k:k + 1], cond=True)
        lat = S.oracle_loop(ora, y[0], False, seeds[k], dev)
        ref = m.decode(lat.unsqueeze(0).to(dev), cond=False)[0]
        err = parity_err(got[k].cpu(), ref.cpu())
        print(f"LBBDM request {k}: {err:.2e}")
        assert err < S.LOOP_TOL, (k, err)
