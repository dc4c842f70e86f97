"""Drop-in check of bbdm_amd's model classes under the reference's training runner, self-contained: what ``BBDMRunner`` does with the
model (runners/BaseRunner.py, runners/DiffusionBasedModelRunners/BBDMRunner.py, runners/utils.py and runners/base/EMA.py of the
reference), restated below and driven through everything that does not need a GPU: construction + ``apply(weights_init)`` (through
the model's overridden ``apply``), optimizer / scheduler creation from ``get_parameters()``, EMA register / update / ``apply_shadow``
/ ``restore``, checkpoint save -> strict load round trip.  (Forward / sampling need the MI355X and are covered by the ``-m gpu``
tests against the oracle.)  The configuration is the model section of the reference's configs/Template-BBDM.yaml, with the UNet
shrunk."""
import argparse

import torch
import torch.nn as nn

import bbdm_amd
from optim_cases import reference_ema_class

# configs/Template-BBDM.yaml, model section (UNetParams shrunk: image_size, model_channels, channel_mult, attention_resolutions,
# num_head_channels); EMA from the first step on
MODEL = {
    "model_name": "BrownianBridge", "model_type": "BBDM", "latent_before_quant_conv": False, "normalize_latent": False,
    "only_load_latent_mean_std": False,
    "EMA": {"use_ema": True, "ema_decay": 0.995, "update_ema_interval": 1, "start_ema_step": 0},
    "CondStageParams": {"n_stages": 2, "in_channels": 3, "out_channels": 3},
    "BB": {
        "optimizer": {"weight_decay": 0.0, "optimizer": "Adam", "lr": 1e-4, "beta1": 0.9},
        "lr_scheduler": {"factor": 0.5, "patience": 3000, "threshold": 0.0001, "cooldown": 3000, "min_lr": 5e-7},
        "params": {
            "mt_type": "linear", "objective": "grad", "loss_type": "l1", "skip_sample": True, "sample_type": "linear",
            "sample_step": 200, "num_timesteps": 1000, "eta": 1.0, "max_var": 1.0,
            "UNetParams": {"image_size": 16, "in_channels": 6, "model_channels": 32, "out_channels": 3, "num_res_blocks": 2,
                           "attention_resolutions": (2,), "channel_mult": (1, 2), "conv_resample": True, "dims": 2,
                           "num_heads": 8, "num_head_channels": 32, "use_scale_shift_norm": True, "resblock_updown": True,
                           "use_spatial_transformer": False, "context_dim": None, "condition_key": "SpatialRescaler"}}},
}


def _ns(c):
    ns = argparse.Namespace()
    for k, v in c.items():
        setattr(ns, k, _ns(v) if isinstance(v, dict) else v)
    return ns


def weights_init(m):
    """runners/utils.py:35-45: N(0, 0.02) on the weights of every module whose class name names Conv2d / Linear / Parameter,
    N(1, 0.02) and 0 on BatchNorm."""
    name = m.__class__.__name__
    if "Conv2d" in name or "Linear" in name or "Parameter" in name:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif "BatchNorm" in name:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class Runner:
    """BBDMRunner(config) as far as the model is concerned: BaseRunner.py:28-80 with BBDMRunner.py:21-29 (model + weights_init) and
    59-68 (get_optimizer's Adam over get_parameters(), ReduceLROnPlateau), EMA registration, the checkpoint load of
    BaseRunner.py:111-138 and the states of BaseRunner.py:140-170 (no DDP, one device)."""

    def __init__(self, config):
        self.config = config
        self.global_epoch, self.global_step = 0, 0
        self.net = bbdm_amd.BrownianBridgeModel(config.model).to(config.training.device[0])
        self.net.apply(weights_init)
        opt, sch = config.model.BB.optimizer, config.model.BB.lr_scheduler
        self.optimizer = [torch.optim.Adam(self.net.get_parameters(), lr=opt.lr, weight_decay=opt.weight_decay, betas=(opt.beta1, 0.999))]
        self.scheduler = [torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer=self.optimizer[0], mode="min", threshold_mode="rel",
                                                                     **vars(sch))]
        self.ema = reference_ema_class()(config.model.EMA.ema_decay)
        self.ema.register(self.net)
        self.load_model_from_checkpoint()

    def load_model_from_checkpoint(self):
        path = getattr(self.config.model, "model_load_path", None)
        if path is None:
            return
        states = torch.load(path, map_location="cpu")
        self.global_epoch, self.global_step = states["epoch"], states["step"]
        self.net.load_state_dict(states["model"])           # strict
        self.ema.shadow = states["ema"]

    def get_checkpoint_states(self):
        model_states = {"step": self.global_step, "model": self.net.state_dict(), "epoch": self.global_epoch + 1,
                        "ema": self.ema.shadow}
        return model_states, {"optimizer": [o.state_dict() for o in self.optimizer],
                              "scheduler": [s.state_dict() for s in self.scheduler]}


def test_reference_runner_drives_bbdm_amd_model(tmp_path):
    config = _ns({"model": MODEL})
    config.training = argparse.Namespace(use_DDP=False, device=[torch.device("cpu")], local_rank=0)

    torch.manual_seed(11)
    runner = Runner(config)
    net = runner.net
    assert isinstance(net, bbdm_amd.BrownianBridgeModel)
    # weights_init reached every Conv2d / Linear through the overridden apply(): zero_module convs are re-initialised,
    # the Conv1d proj_out of the attention block stays zero
    sd = net.state_dict()
    assert float(sd["denoise_fn.out.2.weight"].abs().max()) > 0
    proj = [k for k in sd if k.endswith("proj_out.weight")]
    assert proj and all(float(sd[k].abs().max()) == 0 for k in proj)
    # optimizer over get_parameters(), scheduler
    assert len(runner.optimizer) == 1 and len(runner.scheduler) == 1
    n_opt = sum(p.numel() for g in runner.optimizer[0].param_groups for p in g["params"])
    assert n_opt == sum(p.numel() for p in net.denoise_fn.parameters())
    # EMA: register / update / apply_shadow / restore work on our parameter names
    ema = runner.ema
    assert set(ema.shadow) == {k for k, p in net.named_parameters() if p.requires_grad}
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.01)
    ema.update(net, with_decay=True)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    ema.apply_shadow(net)
    assert any(not torch.equal(before[k], p) for k, p in net.named_parameters())
    ema.restore(net)
    assert all(torch.equal(before[k], p) for k, p in net.named_parameters())
    # checkpoint round trip through the runner's state-dict plumbing (strict load)
    runner.global_step = 5
    model_states, optim_states = runner.get_checkpoint_states()
    path = tmp_path / "ckpt.pth"
    torch.save(model_states, path)
    config.model.model_load_path = str(path)
    fresh = Runner(config)
    for k, v in net.state_dict().items():
        assert torch.equal(fresh.net.state_dict()[k], v), k
    assert fresh.global_step == runner.global_step
    assert all(torch.equal(fresh.ema.shadow[k], v) for k, v in ema.shadow.items())
