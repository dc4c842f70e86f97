"""Golden fixture of the small reference-parity checks, produced by the REAL reference checkout.

TEST INFRASTRUCTURE.  Run wherever the reference checkout is at hand (it is needed here only, never by the tests):

    python oracle/make_golden_refparity.py REFERENCE_CHECKOUT      ->  tests/golden/ref_parity.pt

Stored, per check (each one the reference side of a test that used to import the checkout itself):
  first_stage : tests/test_first_stage.py -- the reference's VQModel (model/VQGAN/vqgan.py, pytorch_lightning stubbed) at three
                small geometries: its state_dict layout (key order and shapes; the test draws the shared weights from them), and
                encode -> quantize -> decode -> forward on the test's input under those weights;
  cond_stage  : tests/test_cond_stage.py -- the reference's SpatialRescaler (model/BrownianBridge/base/modules/encoders/modules.py)
                for every case of the test: its seeded state_dict, the input, forward and encode outputs;
  fresh_init  : tests/test_abi.py -- the reference's BrownianBridgeModel built under torch.manual_seed(7) at the tiny_concat
                golden geometry: its seeded initial state_dict as key order, dtype, shape and sha256 of the bytes of every tensor
                (the 4 M values themselves would be 18 MB).
"""
from __future__ import annotations

import argparse
import hashlib
import importlib
import importlib.machinery
import os
import sys
import types

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TESTS = os.path.join(ROOT, "tests")
OUT = os.path.join(TESTS, "golden", "ref_parity.pt")


def _ns(c):
    ns = argparse.Namespace()
    for k, v in c.items():
        setattr(ns, k, _ns(v) if isinstance(v, dict) else v)
    return ns


def first_stage():
    sys.path[:0] = [TESTS]
    from test_first_stage import CASES, vq_params, shared_weights
    pl = types.ModuleType("pytorch_lightning")
    pl.__spec__ = importlib.machinery.ModuleSpec("pytorch_lightning", None)
    pl.LightningModule = nn.Module
    sys.modules.setdefault("pytorch_lightning", pl)
    from model.VQGAN.vqgan import VQModel as RefVQ
    out = {}
    for attn, with_conv in CASES:
        torch.manual_seed(0)
        ref = RefVQ(**vars(_ns(vq_params(attn, with_conv)))).eval()
        shapes = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        sd, x = shared_weights(shapes)
        ref.load_state_dict(sd, strict=True)
        with torch.no_grad():
            za = ref.quant_conv(ref.encoder(x))
            qa, la, ia = ref.quantize(za)
            out[(tuple(attn), with_conv)] = {"shapes": shapes, "z": za, "q": qa, "loss": float(la), "idx": ia[2].reshape(-1),
                                             "dec": ref.decode(qa), "fwd": ref(x)[0]}
    return out


def cond_stage():
    sys.path[:0] = [TESTS]
    from test_cond_stage import CASES
    ref_cls = importlib.import_module("model.BrownianBridge.base.modules.encoders.modules").SpatialRescaler
    out = []
    for kw in CASES:
        torch.manual_seed(1)
        ref = ref_cls(**kw)
        x = torch.randn(2, kw["in_channels"], 16, 24)
        with torch.no_grad():
            out.append({"kw": kw, "state_dict": ref.state_dict(), "x": x, "fwd": ref(x), "enc": ref.encode(x)})
    return out


def fresh_init():
    sys.path[:0] = [TESTS, HERE]
    from fixtures import load_case
    from model.BrownianBridge.BrownianBridgeModel import BrownianBridgeModel as Ref
    rec = load_case("tiny_concat")
    torch.manual_seed(7)
    a = Ref(_ns({"BB": {"params": dict(rec["bb_params"], UNetParams=rec["unet_params"])}}))
    return {"case": "tiny_concat", "seed": 7, "state_dict": [(k, str(v.dtype), tuple(v.shape), tensor_sha256(v))
                                                             for k, v in a.state_dict().items()]}


def tensor_sha256(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="the reference checkout (the directory that holds model/ and runners/)")
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.reference), ROOT]
    rec = {"first_stage": first_stage(), "cond_stage": cond_stage(), "fresh_init": fresh_init()}
    torch.save(rec, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
