"""Shared bodies of the gradient-clipping / non-finite-guard tests of bbdm_amd.optim (run on the GPU by test_optim_clip_gpu.py and
on the CPU-emulated kernels by test_optim_clip_emu_cpu.py): FusedAdam(max_grad_norm=, skip_nonfinite=), grad_norm and
clip_grad_norm_ against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam and against fp64 sums on the host.

The net is optim_cases.make_net: 8 tensors, 51 990 parameters, odd sizes (unaligned chunk starts, tails, one tensor of 49 950
elements = 4 chunks, a 3-element bias) -- 11 chunks in all."""
import argparse

import pytest
import torch

from optim_cases import make_net, rel

# Parity tolerances: adam_parity's (optim_cases.py), unchanged.  torch forms the norm in fp32 in another order than the kernel's fp64 sum,
# and that rounding enters every clipped gradient through the coefficient.  What it moves was measured as the issue prescribes -- the
# SAME torch path (the six steps of parity() below) once with torch's fp32 norm and once with the norm summed in fp64 and rounded to
# fp32 (measure_torch_norm_rounding() below, CPU): coefficient 3.3e-7, parameters 1.3e-7, exp_avg 2.5e-7 / 4.5e-7 and exp_avg_sq
# 6.3e-7 / 5.0e-7 without / with weight decay (on the GPU, whose fp32 norm is summed in another order again: 1.3e-7, 1.3e-7, 1.4e-7 /
# 1.6e-7, 2.3e-7 / 2.7e-7; profiles/optim_clip.txt).  torch's rounding alone stays below adam_parity's tolerances, so they are not widened.
TOL_P = {0.0: 1e-6, 0.01: 3e-6}       # parameters: without / with weight decay (see adam_parity)
TOL_M = 1e-6                          # both moments
TOL_NORM = 1e-6                       # returned norm against torch's fp32 norm (which itself is within ~1e-7 of the fp64 sum)


def set_grads(nets, gen, scale, dev):
    """The same fresh gradients (randn * scale) on every net of ``nets``."""
    for ps in zip(*(n.parameters() for n in nets)):
        gr = (torch.randn(ps[0].shape, generator=gen) * scale).to(dev)
        for p in ps:
            p.grad = gr.clone()


def host_norm64(params):
    return float(torch.sqrt(sum((p.grad.detach().cpu().double() ** 2).sum() for p in params if p.grad is not None)))


def torch_clip(params, max_norm, norm64):
    """torch.nn.utils.clip_grad_norm_, or the same with the norm summed in fp64 and rounded to fp32 (the tolerance measurement)."""
    params = list(params)
    if not norm64:
        return torch.nn.utils.clip_grad_norm_(params, max_norm)
    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params if p.grad is not None)).float()
    torch.nn.utils.clip_grads_with_norm_(params, max_norm, total)
    return total


def parity(dev, wd, beta1=None, check=True, norm64=False, net_b=None):
    """Case 1: six steps, gradients 1e-3 .. 1e2, max_grad_norm = 1: the first step does not clip (norm 0.23), the others do."""
    from bbdm_amd.optim import FusedAdam
    beta1 = beta1 if beta1 is not None else (0.9 if wd == 0.0 else 0.5)
    a, b = make_net(1, dev), make_net(1, dev)
    oa = FusedAdam(a.parameters(), lr=1e-3, betas=(beta1, 0.999), weight_decay=wd, max_grad_norm=1.0)
    ob = torch.optim.Adam(b.parameters(), lr=1e-3, betas=(beta1, 0.999), weight_decay=wd)
    g = torch.Generator().manual_seed(5)
    coefs = []
    for it in range(6):
        set_grads((a, b), g, 10.0 ** (it - 3), dev)
        if it == 3:                                   # a parameter without a gradient: not in the norm, no update -- in both
            a[2].bias.grad = b[2].bias.grad = None
        if it == 4:
            for o in (oa, ob):
                o.param_groups[0]["lr"] = 3e-4
        grads_before = [None if p.grad is None else p.grad.clone() for p in a.parameters()]
        oa.step()
        for p, g0 in zip(a.parameters(), grads_before):          # clipping happens inside the pass: p.grad is not rescaled
            assert g0 is None or torch.equal(p.grad, g0)
        norm_b = torch_clip(b.parameters(), 1.0, norm64)
        ob.step()
        coefs.append(float(torch.clamp(1.0 / (norm_b + 1e-6), max=1.0)))
        if check:
            tol = TOL_P[wd]
            print(f"step {it}: norm fused {float(oa.grad_norm):.9g} torch {float(norm_b):.9g} "
                  f"rel {abs(float(oa.grad_norm) - float(norm_b)) / float(norm_b):.2e}; worst parameter rel "
                  f"{max(rel(pa, pb) for pa, pb in zip(a.parameters(), b.parameters())):.2e}")
            assert oa.grad_norm.dim() == 0 and oa.grad_norm.dtype == torch.float32 and oa.grad_norm.device == a[0].weight.device
            assert abs(float(oa.grad_norm) - float(norm_b)) <= TOL_NORM * float(norm_b), it
            for (k, pa), pb in zip(a.named_parameters(), b.parameters()):
                assert rel(pa, pb) < tol, (it, k, rel(pa, pb))
    assert coefs[0] == 1.0 and all(c < 1.0 for c in coefs[1:])      # some steps clip, one does not
    sa, sb = oa.state_dict(), ob.state_dict()
    if check:
        for i in sa["state"]:
            assert float(sa["state"][i]["step"]) == float(sb["state"][i]["step"])
            assert rel(sa["state"][i]["exp_avg"], sb["state"][i]["exp_avg"]) < TOL_M
            assert rel(sa["state"][i]["exp_avg_sq"], sb["state"][i]["exp_avg_sq"]) < TOL_M
    return b, sb, coefs


def measure_torch_norm_rounding(dev=torch.device("cpu")):
    """What torch's fp32 norm alone moves, on parity()'s inputs (see the note at TOL_P): printed, not asserted."""
    for wd in (0.0, 0.01):
        b32, s32, c32 = parity(dev, wd, check=False, norm64=False)
        b64, s64, c64 = parity(dev, wd, check=False, norm64=True)
        print(f"wd={wd}: coef {max(abs(x - y) / y for x, y in zip(c32, c64)):.2e} "
              f"param {max(rel(p, q) for p, q in zip(b32.parameters(), b64.parameters())):.2e} "
              f"exp_avg {max(rel(s32['state'][i]['exp_avg'], s64['state'][i]['exp_avg']) for i in s32['state']):.2e} "
              f"exp_avg_sq {max(rel(s32['state'][i]['exp_avg_sq'], s64['state'][i]['exp_avg_sq']) for i in s32['state']):.2e}")


def standalone_clip_parity(dev):
    """clip_grad_norm_ (norm pass, finalize, scale pass) against torch's, clipping and not clipping; step(max_grad_norm=) override."""
    from bbdm_amd.optim import FusedAdam, clip_grad_norm_
    a, b = make_net(3, dev), make_net(3, dev)
    g = torch.Generator().manual_seed(11)
    for scale, max_norm in ((1e-2, 0.5), (1e-4, 0.5), (3.0, 2.0)):
        set_grads((a, b), g, scale, dev)
        na = clip_grad_norm_(a.parameters(), max_norm)
        nb = torch.nn.utils.clip_grad_norm_(b.parameters(), max_norm)
        assert na.dim() == 0 and na.dtype == torch.float32 and na.device == nb.device
        assert abs(float(na) - float(nb)) <= TOL_NORM * float(nb)
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert rel(pa.grad, pb.grad) < 1e-6
    # the per-call override: an optimizer built without clipping, clipped for one step
    set_grads((a, b), g, 1.0, dev)
    oa, ob = FusedAdam(a.parameters(), lr=1e-3), torch.optim.Adam(b.parameters(), lr=1e-3)
    assert oa.max_grad_norm is None and oa.grad_norm is None
    oa.step(max_grad_norm=0.25)
    torch.nn.utils.clip_grad_norm_(b.parameters(), 0.25)
    ob.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert rel(pa, pb) < 1e-6
    assert oa.max_grad_norm is None


def norm_accuracy(dev):
    """Case 2: relative error <= 1e-6 against an fp64 sum for total norms of about 1e-8, 1e-3, 1 and 1e4."""
    from bbdm_amd.optim import grad_norm
    net = make_net(4, dev)
    g = torch.Generator().manual_seed(13)
    set_grads((net,), g, 1.0, dev)
    base = [p.grad.clone() for p in net.parameters()]
    n0 = host_norm64(net.parameters())
    for target in (1e-8, 1e-3, 1.0, 1e4):
        for p, b in zip(net.parameters(), base):
            p.grad = b * (target / n0)
        want = host_norm64(net.parameters())
        got = grad_norm(net.parameters())
        err = abs(float(got.double()) - want) / want
        print(f"norm {want:.6e}: rel err {err:.2e}")
        assert 0.5 * target < want < 2 * target
        assert err <= 1e-6, (target, err)


def norm_window(dev):
    """Case 2: the window is per chunk, sum of squares < 2^32 (csrc/optim.hip).  Just inside is exact, outside is NaN, as Inf / NaN are."""
    from bbdm_amd.optim import grad_norm
    net = make_net(4, dev)
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    w = net[3].weight
    w.grad.view(-1)[20000] = 65000.0                 # second chunk of the large tensor: 65000^2 < 2^32
    net[0].bias.grad[5] = 3.0
    want = (65000.0 ** 2 + 9.0) ** 0.5
    assert abs(float(grad_norm(net.parameters())) - want) <= 1e-6 * want
    for bad in (66000.0, 1e30, float("inf"), float("-inf"), float("nan")):
        w.grad.view(-1)[20000] = bad
        assert torch.isnan(grad_norm(net.parameters())), bad
    w.grad.view(-1)[20000] = 1.0                     # and the cells carry nothing over from the previous call
    assert abs(float(grad_norm(net.parameters())) - 10.0 ** 0.5) <= 1e-6 * 10.0 ** 0.5


def order_independence(dev):
    """Case 3: reversed parameter order (other table rows, other cells) and a repeated call give the same norm bit for bit."""
    from bbdm_amd.optim import FusedAdam, grad_norm
    net = make_net(5, dev)
    g = torch.Generator().manual_seed(17)
    set_grads((net,), g, 0.37, dev)
    params = list(net.parameters())
    n1 = grad_norm(params).clone()
    n2 = grad_norm(params).clone()
    n3 = grad_norm(params[::-1]).clone()
    n4 = grad_norm(params[3:] + params[:3]).clone()
    bits = [int(n.view(torch.int32)) for n in (n1, n2, n3, n4)]
    assert bits[0] == bits[1] == bits[2] == bits[3], bits
    # the optimizer's own norm pass: two parameter groups in another order -> two tables -> the same bits again
    opt = FusedAdam([{"params": params[5:]}, {"params": params[:5]}], lr=0.0, max_grad_norm=1.0)
    opt.step()
    assert int(opt.grad_norm.view(torch.int32)) == bits[0]
    assert abs(float(n1) - host_norm64(params)) <= 1e-6 * host_norm64(params)


def loose_bound_is_identity(dev):
    """Case 4: max_grad_norm = 1e30 -> coef == 1.0f exactly -> the bits of the unclipped step (weight decay and EMA included)."""
    from bbdm_amd.optim import EMA, FusedAdam
    a, b = make_net(6, dev), make_net(6, dev)
    ea, eb = EMA(0.995), EMA(0.995)
    ea.register(a); eb.register(b)
    oa = FusedAdam(a.parameters(), lr=1e-3, weight_decay=0.01, max_grad_norm=1e30)
    ob = FusedAdam(b.parameters(), lr=1e-3, weight_decay=0.01)
    g = torch.Generator().manual_seed(19)
    for it in range(3):
        set_grads((a, b), g, 10.0 ** (it - 1), dev)
        oa.step(ema=ea)
        ob.step(ema=eb)
    assert float(oa.skipped_steps) == 0
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    for (k, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(pa, pb), k
        assert torch.equal(ea.shadow[k], eb.shadow[k]), k
    for i in sa:
        assert torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"])


def guard(dev, bad):
    """Case 5: one Inf / NaN in one gradient."""
    from bbdm_amd.optim import EMA, FusedAdam
    a, b = make_net(7, dev), make_net(7, dev)        # b: the same steps without the guard, its step counter advanced by hand
    ema = EMA(0.9)
    ema.register(a)
    oa = FusedAdam(a.parameters(), lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    ob = FusedAdam(b.parameters(), lr=1e-3, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(23)
    set_grads((a, b), g, 1.0, dev)
    oa.step(); ob.step()                              # a clean step first: the moments are not zero
    assert int(oa.skipped_steps) == 0
    set_grads((a,), g, 1.0, dev)
    a[3].weight.grad.view(-1)[17000] = bad
    p0 = {k: p.detach().clone() for k, p in a.named_parameters()}
    s0 = {i: (s["exp_avg"].clone(), s["exp_avg_sq"].clone()) for i, s in oa.state_dict()["state"].items()}
    sh0 = {k: v.clone() for k, v in ema.shadow.items()}
    oa.step(ema=ema, ema_with_decay=True)
    assert torch.isnan(oa.grad_norm)
    assert oa.skipped_steps.dtype == torch.int64 and oa.skipped_steps.device == a[0].weight.device and int(oa.skipped_steps) == 1
    for k, p in a.named_parameters():
        assert torch.equal(p, p0[k]), k
        want = (1.0 - 0.9) * p0[k] + 0.9 * sh0[k]                                    # the fused EMA update is still applied
        assert not torch.equal(ema.shadow[k], sh0[k]) and rel(ema.shadow[k], want) < 1e-6, k
    for i, s in oa.state_dict()["state"].items():
        assert torch.equal(s["exp_avg"], s0[i][0]) and torch.equal(s["exp_avg_sq"], s0[i][1])
        assert float(s["step"]) == 2.0               # the host-side counter advances on a skipped step (documented)
    for p in b.parameters():                         # the twin: no update, the counter bumped as the skipped step bumped it
        ob.state[p]["step"] += 1
    set_grads((a, b), g, 1.0, dev)
    oa.step(); ob.step()                              # the next clean step updates normally
    assert int(oa.skipped_steps) == 1
    for (k, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(pa, pb) and not torch.equal(pa, p0[k]), k
        assert bool(torch.isfinite(pa).all())


def no_guard_propagates(dev, bad):
    """Case 5: the same input with skip_nonfinite=False: the parameters become non-finite, as torch's do."""
    from bbdm_amd.optim import FusedAdam
    a, b = make_net(7, dev), make_net(7, dev)
    oa = FusedAdam(a.parameters(), lr=1e-3, max_grad_norm=1.0)
    ob = torch.optim.Adam(b.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(23)
    set_grads((a, b), g, 1.0, dev)
    for n in (a, b):
        n[3].weight.grad.view(-1)[17000] = bad
    oa.step()
    torch.nn.utils.clip_grad_norm_(b.parameters(), 1.0)
    ob.step()
    assert not bool(torch.isfinite(b[3].weight).all())               # torch: at least the element that held the Inf / NaN
    assert not bool(torch.isfinite(a[3].weight).all())
    assert float(oa.skipped_steps) == 0                               # nothing was skipped, nothing counted


def interface(dev):
    """Case 6 (everything that needs one device)."""
    import bbdm_amd.optim as O
    net = make_net(8, dev)
    opt = O.FusedAdam(net.parameters(), lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True)
    assert opt.max_grad_norm == 0.5 and opt.skip_nonfinite is True
    for key in ("max_grad_norm", "skip_nonfinite"):                  # attributes, NOT hyper-parameters of the groups
        assert key not in opt.param_groups[0] and key not in opt.defaults and key not in opt.state_dict()["param_groups"][0]
    g = torch.Generator().manual_seed(29)
    set_grads((net,), g, 1.0, dev)
    net[2].bias.grad = None                          # a parameter without a gradient is left out of the norm, as torch leaves it out
    want = host_norm64(net.parameters())
    assert abs(float(O.grad_norm(net.parameters())) - want) <= 1e-6 * want
    assert abs(float(torch.nn.utils.clip_grad_norm_(net.parameters(), 1e9)) - want) <= 1e-6 * want
    opt.step()
    assert abs(float(opt.grad_norm) - want) <= 1e-6 * want
    # state_dict round trip with torch.optim.Adam in both directions
    net_t = make_net(8, dev)
    for p, q in zip(net.parameters(), net_t.parameters()):
        q.grad = None if p.grad is None else p.grad.clone()
    opt_t = torch.optim.Adam(net_t.parameters(), lr=1e-3)
    opt_t.step()
    sd, sd_t = opt.state_dict(), opt_t.state_dict()
    assert sd["state"].keys() == sd_t["state"].keys()
    opt.load_state_dict(sd_t)
    opt_t.load_state_dict(sd)
    assert opt.max_grad_norm == 0.5 and opt.skip_nonfinite is True     # loading a checkpoint does not touch the attributes
    opt.step(); opt_t.step()
    # get_optimizer: the keys from a namespace; their absence = off
    cfg = argparse.Namespace(optimizer="Adam", lr=1e-4, weight_decay=0.0, beta1=0.9)
    o1 = O.get_optimizer(cfg, make_net(8, dev).parameters())
    assert isinstance(o1, O.FusedAdam) and o1.max_grad_norm is None and o1.skip_nonfinite is False
    cfg.max_grad_norm, cfg.skip_nonfinite = 2.5, True
    o2 = O.get_optimizer(cfg, make_net(8, dev).parameters())
    assert o2.max_grad_norm == 2.5 and o2.skip_nonfinite is True
    # only the L2 norm
    for fn in (lambda: O.grad_norm(net.parameters(), norm_type=1.0), lambda: O.clip_grad_norm_(net.parameters(), 1.0, norm_type=float("inf")),
               lambda: O.clip_grad_norm_(net.parameters(), 1.0, 3)):
        with pytest.raises(NotImplementedError):
            fn()
    with pytest.raises(ValueError):
        O.FusedAdam(net.parameters(), max_grad_norm=-1.0)
