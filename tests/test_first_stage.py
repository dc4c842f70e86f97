"""bbdm_amd.first_stage.VQModel (PyTorch first stage) against the reference's VQModel on the CPU: identical state_dict
layout, identical encode / quantise / decode results under shared weights.  The reference side is stored in
tests/golden/ref_parity.pt (oracle/make_golden_refparity.py)."""
import argparse
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_parity.pt")
CASES = [((16,), True), ((), True), ((8, 16), False)]


def _ns(c):
    ns = argparse.Namespace()
    for k, v in c.items():
        setattr(ns, k, _ns(v) if isinstance(v, dict) else v)
    return ns


def vq_params(attn, with_conv):
    dd = dict(double_z=False, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2, 2),
              num_res_blocks=2, attn_resolutions=list(attn), dropout=0.0, resamp_with_conv=with_conv)
    return dict(ckpt_path=None, embed_dim=4, n_embed=64, ddconfig=dd, lossconfig={"target": "torch.nn.Identity"})


def shared_weights(shapes):
    """The weights both sides load (drawn in the reference's state_dict order) and the input images."""
    g = torch.Generator().manual_seed(1)
    sd = {k: (torch.randn(s, generator=g) * (0.3 if "embedding" in k else 0.05) + (1.0 if "norm" in k and k.endswith("weight") else 0.0))
          for k, s in shapes}
    x = torch.randn(2, 3, 32, 32, generator=g).clamp(-1, 1)
    return sd, x


@pytest.mark.parametrize("attn,with_conv", CASES)
def test_first_stage_matches_reference(attn, with_conv):
    from bbdm_amd.first_stage import VQModel
    ref = torch.load(GOLDEN, weights_only=False)["first_stage"][(tuple(attn), with_conv)]
    torch.manual_seed(0)
    ours = VQModel(**vars(_ns(vq_params(attn, with_conv)))).eval()
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == dict(ref["shapes"])
    sd, x = shared_weights(ref["shapes"])
    ours.load_state_dict(sd, strict=True)
    with torch.no_grad():
        za, zb = ref["z"], ours.quant_conv(ours.encoder(x))
        assert float((za - zb).abs().max()) < 1e-5 * float(za.abs().max())
        qb, lb, ib = ours.quantize(za)
        assert torch.equal(ref["idx"], ib[2].reshape(-1)) and torch.equal(ref["q"], qb)
        assert abs(ref["loss"] - float(lb)) < 1e-7
        da, db = ref["dec"], ours.decode(ref["q"])
        assert float((da - db).abs().max()) < 2e-5 * float(da.abs().max())
        ra, rb = ref["fwd"], ours(x)
        assert float((ra - rb[0]).abs().max()) < 5e-4 * float(ra.abs().max())
