"""Gradient-norm clipping and the non-finite guard of bbdm_amd.optim on the GPU (bodies: tests/optim_clip_cases.py), and the clipped
step at the real 237 M-parameter size: parity with torch.nn.utils.clip_grad_norm_ + torch.optim.Adam, and its time printed next to the
unclipped fused step's and torch's."""
import pytest
import torch

import optim_clip_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_clipped_fused_adam_matches_torch_clip_and_adam(dev, wd):
    C.parity(dev, wd)


def test_clip_grad_norm_matches_torch_and_step_override(dev):
    C.standalone_clip_parity(dev)


def test_norm_accuracy_against_fp64(dev):
    C.norm_accuracy(dev)


def test_norm_window(dev):
    C.norm_window(dev)


def test_norm_is_order_independent(dev):
    C.order_independence(dev)


def test_loose_bound_is_bitwise_identity(dev):
    C.loose_bound_is_identity(dev)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_guard_skips_the_step(dev, bad):
    C.guard(dev, bad)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_without_guard_nonfinite_propagates(dev, bad):
    C.no_guard_propagates(dev, bad)


def test_interface(dev):
    C.interface(dev)


def test_parameters_on_two_devices_raise(dev):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from bbdm_amd.optim import FusedAdam, clip_grad_norm_
    a, b = torch.nn.Parameter(torch.ones(5, device="cuda:0")), torch.nn.Parameter(torch.ones(7, device="cuda:1"))
    a.grad, b.grad = torch.ones_like(a), torch.ones_like(b)
    opt = FusedAdam([a, b], lr=1e-3, max_grad_norm=1.0)
    with pytest.raises(ValueError):
        opt.step()
    assert len(opt.state) == 0 and bool((a == 1).all()) and bool((b == 1).all())      # raised before anything was touched
    with pytest.raises(ValueError):
        clip_grad_norm_([a, b], 1.0)
    opt.step(max_grad_norm=None)                    # unclipped, two devices stay what they were: one launch per device


def _ms(fn, reps=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def test_full_size_clipped_step_parity_and_time(dev):
    """All 248 tensors / 237 M parameters (~14 500 chunks) of the Template UNet, gradient norm 15.4 clipped to 1: parameters, moments,
    the EMA shadow and the norm against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (foreach) + the EMA formula, to case 1's
    tolerances; the norm against an fp64 sum to 1e-6.  Prints the time per step of the clipped fused step, of the unclipped fused step
    and of torch's clip + Adam; asserts only that the clipped fused step is not slower than torch's (what ~14 500 workgroups meeting on
    one atomic address would make it)."""
    import bench
    import bbdm_amd
    from bbdm_amd.optim import EMA, FusedAdam
    up = bench.WORKLOADS["c4"][1]
    net = bbdm_amd.unet.UNetModel(**up).to(dev)
    ref = bbdm_amd.unet.UNetModel(**up).to(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    for p, q in zip(net.parameters(), ref.parameters()):
        p.data.normal_(0, 0.02, generator=g)
        q.data.copy_(p.data)
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
        q.grad = p.grad.clone()
    want = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in net.parameters())))
    ema = EMA(0.995)
    ema.register(net)
    shadow_ref = {k: v.clone() for k, v in ema.shadow.items()}
    opt = FusedAdam(net.parameters(), lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-4)
    for it in range(3):
        opt.step(ema=ema, ema_with_decay=True)
        for p, q in zip(net.parameters(), ref.parameters()):      # torch rescales .grad in place; the fused pass leaves it alone
            q.grad.copy_(p.grad)
        norm_ref = torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        opt_ref.step()
        for k, q in ref.named_parameters():
            shadow_ref[k] = (1.0 - 0.995) * q.data + 0.995 * shadow_ref[k]
    torch.cuda.synchronize()
    got = float(opt.grad_norm)
    worst = worst_m = 0.0
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        worst = max(worst, C.rel(p.data, q.data), C.rel(ema.shadow[k], shadow_ref[k]))
        worst_m = max(worst_m, C.rel(opt.state[p]["exp_avg"], opt_ref.state[q]["exp_avg"]),
                      C.rel(opt.state[p]["exp_avg_sq"], opt_ref.state[q]["exp_avg_sq"]))
    n = sum(p.numel() for p in net.parameters())
    ms_clip = _ms(lambda: opt.step(ema=ema, ema_with_decay=True))
    ms_plain = _ms(lambda: opt.step(ema=ema, ema_with_decay=True, max_grad_norm=None, skip_nonfinite=False))

    def torch_step():
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        opt_ref.step()
    ms_torch = _ms(torch_step)
    print(f"{n / 1e6:.1f} M parameters: clipped fused Adam+EMA {ms_clip:.3f} ms/step, unclipped fused Adam+EMA {ms_plain:.3f} ms/step "
          f"(+{ms_clip - ms_plain:.3f} ms for 4 more B per parameter = {4 * n / 1e9:.2f} GB), torch clip_grad_norm_ + Adam {ms_torch:.3f} "
          f"ms/step; norm fused {got:.9g} torch {float(norm_ref):.9g} fp64 {want:.9g}; worst rel err parameters / shadow {worst:.2e} "
          f"moments {worst_m:.2e}")
    assert int(opt.skipped_steps) == 0
    assert abs(got - want) <= 1e-6 * want
    assert abs(got - float(norm_ref)) <= C.TOL_NORM * float(norm_ref)
    assert worst < C.TOL_P[0.0] and worst_m < C.TOL_M
    assert ms_clip <= ms_torch
