"""Shared bodies of the FusedSGD / FusedRMSprop tests of bbdm_amd.optim (run on the GPU by test_optim_rules_gpu.py and on the
CPU-emulated kernels by test_optim_rules_emu_cpu.py).  The yardstick is always torch.optim.SGD / torch.optim.RMSprop (and
torch.nn.utils.clip_grad_norm_, and the reference's EMA class restated in optim_cases.py) stepping a CPU copy of the same net with
the same gradients.

TOL = 1e-6 (max-norm relative, optim_cases.rel) is adam_parity's bar against torch: the kernels repeat torch's operations in
torch's order without FMA contraction, so what is left is the rounding of sqrtf and of the division, and whether an
``a + alpha * b`` is rounded once or twice (ATen's CPU kernels: once) -- a few 6e-8 ulps of the largest element.  With clipping,
torch's fp32 norm (summed in another order than the kernel's fp64 sum) enters every gradient through the coefficient: 3.3e-7 on the
coefficient, below the bar (optim_clip_cases.py's measurement)."""
import argparse
import copy

import pytest
import torch
import torch.nn as nn

from optim_cases import make_net, reference_ema_class, rel

CPU = torch.device("cpu")
TOL = 1e-6

SGD_GRID = [(m, d, n, w) for m in (0.0, 0.9) for d in (0.0, 0.1) for n in (False, True) for w in (0.0, 1e-2)]
RMSPROP_GRID = [(m, w, a) for m in (0.0, 0.9) for w in (0.0, 1e-2) for a in (0.99, 0.9)]
RULES = ["sgd", "rmsprop"]


def make_opts(rule, pa, pb, fused_kw=None, **kw):
    """(fused optimizer over ``pa``, torch's over ``pb``) with the same hyper-parameters; the defaults exercise momentum + decay."""
    from bbdm_amd.optim import FusedRMSprop, FusedSGD
    fused_kw = fused_kw or {}
    if rule == "sgd":
        kw = dict(dict(lr=1e-2, momentum=0.9, weight_decay=1e-2), **kw)
        return FusedSGD(pa, **kw, **fused_kw), (None if pb is None else torch.optim.SGD(pb, **kw))
    kw = dict(dict(lr=1e-3, momentum=0.9, weight_decay=1e-2), **kw)
    return FusedRMSprop(pa, **kw, **fused_kw), (None if pb is None else torch.optim.RMSprop(pb, **kw))


def set_grads(params_on_dev, params_on_cpu, gen, scale):
    """The same fresh gradients (randn * scale, drawn on the CPU) for each parameter list of ``params_on_dev`` and ``params_on_cpu``."""
    lists = [list(ps) for ps in params_on_dev + params_on_cpu]
    for ps in zip(*lists):
        gr = torch.randn(ps[0].shape, generator=gen) * scale
        for p in ps:
            p.grad = gr.to(p.device).clone()


def check_same(pa, oa, pb, ob, tag, tol=TOL):
    """Parameters and EVERY state tensor of the fused optimizer against torch's."""
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert rel(p.detach().cpu(), q.detach()) < tol, (tag, i, "param", rel(p.detach().cpu(), q.detach()))
        sa, sb = oa.state.get(p, {}), ob.state.get(q, {})
        assert {k for k, v in sa.items() if v is not None} == {k for k, v in sb.items() if v is not None}, (tag, i, sa.keys(), sb.keys())
        for k, v in sb.items():
            if v is None:
                continue
            if k == "step":
                assert float(sa[k]) == float(v), (tag, i)
            else:
                assert sa[k].shape == v.shape and rel(sa[k].cpu(), v) < tol, (tag, i, k, rel(sa[k].cpu(), v))


def run_parity(dev, rule, kw, steps=6):
    a, b = make_net(1, dev), make_net(1)
    oa, ob = make_opts(rule, a.parameters(), b.parameters(), **kw)
    g = torch.Generator().manual_seed(5)
    for it in range(steps):
        set_grads([a.parameters()], [b.parameters()], g, 10.0 ** (it - 3))            # spans 1e-3 .. 1e2
        if it == 3:                                   # a parameter without a gradient is skipped by both
            a[2].bias.grad = b[2].bias.grad = None
        if it == 4:                                   # lr changed by a scheduler between steps
            for o in (oa, ob):
                o.param_groups[0]["lr"] *= 0.3
        oa.step()
        ob.step()
        check_same(list(a.parameters()), oa, list(b.parameters()), ob, (rule, kw, it))
    assert oa.state_dict()["state"].keys() == ob.state_dict()["state"].keys()


def sgd_parity(dev, momentum, dampening, nesterov, wd):
    """Case 1.  The invalid corners of the grid raise ValueError, as torch's constructor does."""
    from bbdm_amd.optim import FusedSGD
    kw = dict(momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=wd)
    if nesterov and (momentum <= 0 or dampening != 0):
        net = make_net(1, dev)
        with pytest.raises(ValueError):
            torch.optim.SGD(make_net(1).parameters(), lr=1e-2, **kw)
        with pytest.raises(ValueError):
            FusedSGD(net.parameters(), lr=1e-2, **kw)
        return
    run_parity(dev, "sgd", kw)


def rmsprop_parity(dev, momentum, wd, alpha):
    run_parity(dev, "rmsprop", dict(momentum=momentum, weight_decay=wd, alpha=alpha))


def sgd_first_step_with_dampening(dev):
    """Case 1: the step that creates the momentum buffer writes buf = grad (torch: clone(grad)), NOT momentum * 0 + (1 - dampening) *
    grad; the second step applies the recurrence."""
    a, b = make_net(2, dev), make_net(2)
    oa, ob = make_opts("sgd", a.parameters(), b.parameters(), momentum=0.9, dampening=0.1, weight_decay=0.0)
    g = torch.Generator().manual_seed(31)
    set_grads([a.parameters()], [b.parameters()], g, 1.0)
    oa.step(); ob.step()
    for p, q in zip(a.parameters(), b.parameters()):
        buf = oa.state[p]["momentum_buffer"].cpu()
        assert torch.equal(buf, q.grad) and torch.equal(buf, ob.state[q]["momentum_buffer"])
        assert rel(buf, 0.9 * q.grad) > 0.05
    check_same(list(a.parameters()), oa, list(b.parameters()), ob, "first")
    set_grads([a.parameters()], [b.parameters()], g, 1.0)
    oa.step(); ob.step()
    check_same(list(a.parameters()), oa, list(b.parameters()), ob, "second")


def ragged_params(dev):
    """Case 2 -> (parameters, the storage around the view, a copy of it): sizes 1, 3, 5, chunk - 1, chunk + 1, 2 chunk + 7 and a
    contiguous view that starts 4 bytes into a larger storage (numel % 4 != 0, more than one chunk, data pointer not 16-byte aligned)."""
    from bbdm_amd import _lib
    ce = _lib.load().bbdm_opt_chunk_elems()
    gen = torch.Generator().manual_seed(37)
    params = [nn.Parameter(torch.randn(n, generator=gen).to(dev)) for n in (1, 3, 5, ce - 1, ce + 1, 2 * ce + 7)]
    nview = ce + 4099
    store = torch.randn(1 + nview + 5, generator=gen).to(dev)
    view = store[1:1 + nview]
    assert view.is_contiguous() and view.numel() % 4 != 0 and view.data_ptr() % 16 == 4 and view.data_ptr() == store.data_ptr() + 4
    params.append(nn.Parameter(view))
    assert params[-1].data_ptr() == view.data_ptr()
    return params, store, store.clone()


def ragged(dev, rule, clip):
    """Case 2, plain and through the clipped kernels.  The clipped yardstick is torch's clip with the norm summed in fp64 and rounded
    to fp32 (clip_grads_with_norm_), not clip_grad_norm_'s own fp32 sum: that sum is one ulp (1.2e-7) off the correctly rounded norm
    on these gradients, and on the 1- to 5-element tensors of this case -- where the max-norm bar is a per-element bar and
    g * coef + wd * p cancels -- one ulp of the coefficient becomes 8e-6 of RMSprop's momentum buffer, in torch against torch.
    Clipping against clip_grad_norm_ itself is case 4 (clipping(), on make_net)."""
    pa, store_a, before = ragged_params(dev)
    pb, _, _ = ragged_params(CPU)
    oa, ob = make_opts(rule, pa, pb, fused_kw=dict(max_grad_norm=2.0) if clip else None)
    g = torch.Generator().manual_seed(41)
    for it in range(3):
        set_grads([pa], [pb], g, 0.1 * 3.0 ** it)
        oa.step()
        if clip:
            norm64 = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in pb))
            assert norm64 > 2.0 and abs(float(oa.grad_norm) - float(norm64)) <= TOL * float(norm64)
            torch.nn.utils.clip_grads_with_norm_(pb, 2.0, norm64.float())
        ob.step()
        check_same(pa, oa, pb, ob, (rule, clip, it))
    assert torch.equal(store_a[:1], before[:1]) and torch.equal(store_a[-5:], before[-5:])      # around the view: untouched
    assert not torch.equal(store_a[1:-5], before[1:-5])


def fused_ema(dev, rule):
    """Case 3: step(ema=) == step() then ema.update(net) == the reference's EMA class after torch's step."""
    from bbdm_amd.optim import EMA
    RefEMA = reference_ema_class()
    a, b, c = make_net(2, dev), make_net(2), make_net(2, dev)
    ea, eb, ec = EMA(0.995), RefEMA(0.995), EMA(0.995)
    ea.register(a); eb.register(b); ec.register(c)
    oa, ob = make_opts(rule, a.parameters(), b.parameters())
    oc, _ = make_opts(rule, c.parameters(), None)
    g = torch.Generator().manual_seed(9)
    for it in range(5):
        set_grads([a.parameters(), c.parameters()], [b.parameters()], g, 1.0)
        if it == 3:                                   # no gradient: no update, but the EMA covers every registered parameter
            a[2].bias.grad = b[2].bias.grad = c[2].bias.grad = None
        decay = it >= 2                               # with_decay=False before start_ema_step (BaseRunner.py:174)
        oa.step(); ea.update(a, with_decay=decay)
        ob.step(); eb.update(b, with_decay=decay)
        oc.step(ema=ec, ema_with_decay=decay)
        for k in eb.shadow:
            assert rel(ea.shadow[k].cpu(), eb.shadow[k]) < TOL, (it, k)
            assert rel(ec.shadow[k].cpu(), eb.shadow[k]) < TOL, (it, k)
            assert rel(ec.shadow[k], ea.shadow[k]) < TOL, (it, k)
    for pa, pc in zip(a.parameters(), c.parameters()):
        assert torch.equal(pa, pc)


def clipping(dev, rule, max_norm):
    """Case 4: clipping inside the pass == clip_grad_norm_ + torch's step; p.grad untouched; a bound that never binds (coef == 1.0f)
    gives the bits of the unclipped fused step."""
    a, b, c = make_net(1, dev), make_net(1), make_net(1, dev)
    oa, ob = make_opts(rule, a.parameters(), b.parameters(), fused_kw=dict(max_grad_norm=max_norm))
    oc, _ = make_opts(rule, c.parameters(), None)
    g = torch.Generator().manual_seed(5)
    coefs = []
    for it in range(6):
        set_grads([a.parameters(), c.parameters()], [b.parameters()], g, 10.0 ** (it - 3))
        if it == 3:
            a[2].bias.grad = b[2].bias.grad = c[2].bias.grad = None
        before = [None if p.grad is None else p.grad.clone() for p in a.parameters()]
        oa.step()
        oc.step()
        for p, g0 in zip(a.parameters(), before):
            assert g0 is None or torch.equal(p.grad, g0)
        norm_b = torch.nn.utils.clip_grad_norm_(b.parameters(), max_norm)
        ob.step()
        coefs.append(float(torch.clamp(max_norm / (norm_b + 1e-6), max=1.0)))
        assert abs(float(oa.grad_norm) - float(norm_b)) <= TOL * float(norm_b), it
        check_same(list(a.parameters()), oa, list(b.parameters()), ob, (rule, max_norm, it))
    if max_norm < 1.0:
        assert coefs[0] == 1.0 and all(x < 1.0 for x in coefs[1:])       # one step does not clip, the others do
    else:
        assert all(x == 1.0 for x in coefs)
        for pa, pc in zip(a.parameters(), c.parameters()):
            assert torch.equal(pa, pc)
            for k, v in oc.state[pc].items():
                assert k == "step" or torch.equal(oa.state[pa][k], v), k


def _state_copy(opt):
    return {i: {k: v.clone() for k, v in s.items() if torch.is_tensor(v) and k != "step"} for i, s in opt.state_dict()["state"].items()}


def guard(dev, rule):
    """Case 5: one Inf in one gradient under skip_nonfinite; then a clean step."""
    from bbdm_amd.optim import EMA
    a, b = make_net(7, dev), make_net(7, dev)        # b: the same clean steps on a fused optimizer that never sees the bad one
    ema = EMA(0.9)
    ema.register(a)
    oa, _ = make_opts(rule, a.parameters(), None, fused_kw=dict(max_grad_norm=1.0, skip_nonfinite=True))
    ob, _ = make_opts(rule, b.parameters(), None, fused_kw=dict(max_grad_norm=1.0))
    g = torch.Generator().manual_seed(23)
    set_grads([a.parameters(), b.parameters()], [], g, 1.0)
    oa.step(); ob.step()                              # a clean step first: the state is not zero
    assert int(oa.skipped_steps) == 0
    set_grads([a.parameters()], [], g, 1.0)
    a[3].weight.grad.view(-1)[17000] = float("inf")
    p0 = {k: p.detach().clone() for k, p in a.named_parameters()}
    s0 = _state_copy(oa)
    sh0 = {k: v.clone() for k, v in ema.shadow.items()}
    oa.step(ema=ema, ema_with_decay=True)
    assert torch.isnan(oa.grad_norm)
    assert oa.skipped_steps.dtype == torch.int64 and oa.skipped_steps.device == a[0].weight.device and int(oa.skipped_steps) == 1
    for k, p in a.named_parameters():
        assert torch.equal(p, p0[k]), k
        want = (1.0 - 0.9) * p0[k] + 0.9 * sh0[k]                                    # the fused EMA update is still applied
        assert not torch.equal(ema.shadow[k], sh0[k]) and rel(ema.shadow[k], want) < TOL, k
    s1 = _state_copy(oa)
    assert s1.keys() == s0.keys()
    for i in s0:
        assert s0[i].keys() == ({"momentum_buffer"} if rule == "sgd" else {"momentum_buffer", "square_avg"})
        for k in s0[i]:
            assert torch.equal(s1[i][k], s0[i][k]), (i, k)
    set_grads([a.parameters(), b.parameters()], [], g, 1.0)
    oa.step(); ob.step()                              # the next clean step updates normally
    assert int(oa.skipped_steps) == 1
    for (k, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(pa, pb) and not torch.equal(pa, p0[k]), k
        assert bool(torch.isfinite(pa).all())


def no_guard_propagates(dev, rule):
    """Case 5: without skip_nonfinite the coefficient is NaN and so is every parameter (documented; asserted to keep it deliberate)."""
    a = make_net(7, dev)
    oa, _ = make_opts(rule, a.parameters(), None, fused_kw=dict(max_grad_norm=1.0))
    g = torch.Generator().manual_seed(23)
    set_grads([a.parameters()], [], g, 1.0)
    a[3].weight.grad.view(-1)[17000] = float("inf")
    oa.step()
    for p in a.parameters():
        assert bool(torch.isnan(p).all())
    assert int(oa.skipped_steps) == 0


def sgd_skipped_first_step(dev):
    """Case 5 / the documented divergence: a skipped FIRST step leaves the momentum buffer at zero; for the host the next step is no
    longer the first, so it applies the recurrence: buf = momentum * 0 + (1 - dampening) * grad."""
    a = make_net(7, dev)
    oa, _ = make_opts("sgd", a.parameters(), None, momentum=0.9, dampening=0.1, weight_decay=0.0, fused_kw=dict(skip_nonfinite=True))
    g = torch.Generator().manual_seed(43)
    set_grads([a.parameters()], [], g, 1.0)
    a[0].weight.grad.view(-1)[3] = float("inf")
    p0 = [p.detach().clone() for p in a.parameters()]
    oa.step()
    assert int(oa.skipped_steps) == 1
    for p, q in zip(a.parameters(), p0):
        assert torch.equal(p, q) and not bool(oa.state[p]["momentum_buffer"].any())
    set_grads([a.parameters()], [], g, 1.0)
    oa.step()
    for p in a.parameters():
        assert rel(oa.state[p]["momentum_buffer"], p.grad * 0.9) < TOL
        assert rel(oa.state[p]["momentum_buffer"], p.grad) > 0.05


def reproducible(dev, rule):
    """Case 6: two fresh optimizers, the same gradients, four clipped steps: the same bits."""
    nets = [make_net(3, dev), make_net(3, dev)]
    opts = [make_opts(rule, n.parameters(), None, fused_kw=dict(max_grad_norm=0.5))[0] for n in nets]
    g = torch.Generator().manual_seed(47)
    for it in range(4):
        set_grads([n.parameters() for n in nets], [], g, 10.0 ** (it - 2))
        for o in opts:
            o.step()
    for p, q in zip(nets[0].parameters(), nets[1].parameters()):
        assert torch.equal(p, q)
    assert torch.equal(opts[0].grad_norm, opts[1].grad_norm)


def state_dict_round_trip(dev, rule):
    """Case 7: torch's checkpoint into a fresh fused optimizer and the fused one's into a fresh torch optimizer, one more step: what
    stepping on without the round trip gives."""
    a, b = make_net(4, dev), make_net(4)
    oa, ob = make_opts(rule, a.parameters(), b.parameters())
    g = torch.Generator().manual_seed(53)
    for it in range(2):
        set_grads([a.parameters()], [b.parameters()], g, 1.0)
        oa.step(); ob.step()
    c, d = make_net(4, dev), make_net(4)             # c: fused, from torch's checkpoint;  d: torch, from the fused checkpoint
    c.load_state_dict(b.state_dict())
    d.load_state_dict({k: v.cpu() for k, v in a.state_dict().items()})
    oc, od = make_opts(rule, c.parameters(), d.parameters())
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))            # a checkpoint: load_state_dict itself does not copy tensors that
    od.load_state_dict(copy.deepcopy(oa.state_dict()))            # already have the parameter's device and dtype
    for p in c.parameters():
        assert all(v.device == p.device for k, v in oc.state[p].items() if torch.is_tensor(v) and k != "step")
    set_grads([a.parameters(), c.parameters()], [b.parameters(), d.parameters()], g, 1.0)
    for o in (oa, ob, oc, od):
        o.step()
    check_same(list(a.parameters()), oa, list(b.parameters()), ob, "no round trip")
    check_same(list(c.parameters()), oc, list(b.parameters()), ob, "torch -> fused")
    check_same(list(a.parameters()), oa, list(d.parameters()), od, "fused -> torch")
    if rule == "sgd":                                 # the loaded buffer was USED: a fresh optimizer's first step would give buf = grad
        p = next(iter(c.parameters()))
        assert rel(oc.state[p]["momentum_buffer"], p.grad) > 0.05


def centered_is_refused(dev):
    """Case 7: centered RMSprop (a third state tensor, grad_avg) is refused in the constructor and in a loaded checkpoint."""
    from bbdm_amd.optim import FusedRMSprop
    net, ref = make_net(4, dev), make_net(4)
    with pytest.raises(NotImplementedError):
        FusedRMSprop(net.parameters(), lr=1e-3, centered=True)
    ot = torch.optim.RMSprop(ref.parameters(), lr=1e-3, centered=True)
    set_grads([], [ref.parameters()], torch.Generator().manual_seed(59), 1.0)
    ot.step()
    assert "grad_avg" in ot.state_dict()["state"][0]
    opt = FusedRMSprop(net.parameters(), lr=1e-3)
    with pytest.raises(NotImplementedError):
        opt.load_state_dict(ot.state_dict())


def plateau_scheduler(dev, rule):
    """Case 7: ReduceLROnPlateau lowers param_groups[0]['lr'] and the next step uses it."""
    a, b = make_net(4, dev), make_net(4)
    oa, ob = make_opts(rule, a.parameters(), b.parameters())
    lr0 = oa.param_groups[0]["lr"]
    scheds = [torch.optim.lr_scheduler.ReduceLROnPlateau(o, mode="min", factor=0.25, patience=0) for o in (oa, ob)]
    g = torch.Generator().manual_seed(61)
    for it, loss in enumerate((1.0, 2.0, 3.0)):
        set_grads([a.parameters()], [b.parameters()], g, 1.0)
        oa.step(); ob.step()
        for s in scheds:
            s.step(loss)
        check_same(list(a.parameters()), oa, list(b.parameters()), ob, it)
    assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"] == lr0 * 0.25 ** 2
    before = [p.detach().clone() for p in a.parameters()]
    set_grads([a.parameters()], [b.parameters()], g, 1.0)
    oa.step(); ob.step()
    check_same(list(a.parameters()), oa, list(b.parameters()), ob, "lowered lr")
    assert all(not torch.equal(p, q) for p, q in zip(a.parameters(), before))


def get_optimizer_cases(dev):
    """Case 8 (what needs no real device check)."""
    import bbdm_amd
    import bbdm_amd.optim as O
    cfg = argparse.Namespace(optimizer="RMSProp", lr=2e-4, weight_decay=0.01, beta1=0.9)
    o = O.get_optimizer(cfg, make_net(8, dev).parameters())
    assert type(o) is O.FusedRMSprop and isinstance(o, torch.optim.Optimizer) and bbdm_amd.FusedRMSprop is O.FusedRMSprop
    grp = o.param_groups[0]
    assert (grp["lr"], grp["weight_decay"], grp["alpha"], grp["eps"], grp["momentum"], grp["centered"]) == (2e-4, 0.01, 0.99, 1e-8, 0, False)
    assert o.max_grad_norm is None and o.skip_nonfinite is False
    cfg.optimizer = "SGD"
    o = O.get_optimizer(cfg, make_net(8, dev).parameters())
    assert type(o) is O.FusedSGD and bbdm_amd.FusedSGD is O.FusedSGD
    grp = o.param_groups[0]
    assert (grp["lr"], grp["momentum"], grp["dampening"], grp["weight_decay"], grp["nesterov"]) == (2e-4, 0.9, 0, 0, False)
    assert o.max_grad_norm is None and o.skip_nonfinite is False
    cfg.max_grad_norm, cfg.skip_nonfinite = 2.5, True
    for name, cls in (("RMSProp", O.FusedRMSprop), ("SGD", O.FusedSGD), ("Adam", O.FusedAdam)):
        cfg.optimizer = name
        o = O.get_optimizer(cfg, make_net(8, dev).parameters())
        assert type(o) is cls and o.max_grad_norm == 2.5 and o.skip_nonfinite is True
        for key in ("max_grad_norm", "skip_nonfinite"):              # attributes, NOT hyper-parameters of the groups
            assert key not in o.param_groups[0] and key not in o.defaults and key not in o.state_dict()["param_groups"][0]
        # and the optimizer it returned takes a guarded, clipped step with a fused EMA
        net = make_net(8, dev)
        o = O.get_optimizer(cfg, net.parameters())
        ema = O.EMA(0.9)
        ema.register(net)
        set_grads([net.parameters()], [], torch.Generator().manual_seed(67), 1.0)
        p0 = [p.detach().clone() for p in net.parameters()]
        o.step(ema=ema)
        assert int(o.skipped_steps) == 0 and all(not torch.equal(p, q) for p, q in zip(net.parameters(), p0))
    cfg.optimizer = "Foo"
    with pytest.raises(NotImplementedError):
        O.get_optimizer(cfg, make_net(8, dev).parameters())
    with pytest.raises(ValueError):
        O.FusedSGD(make_net(8, dev).parameters(), max_grad_norm=-1.0)


def cpu_parameters_are_refused():
    """Case 8: no fallback -- CPU parameters raise at step() what FusedAdam raises for them.  Needs the real library (not the
    emulated back end, which is how the other CPU tests get past this very check)."""
    import bbdm_amd.optim as O
    from bbdm_amd._lib import BBDMHipError
    cfg = argparse.Namespace(optimizer="Adam", lr=1e-4, weight_decay=0.0, beta1=0.9)
    for name in ("Adam", "RMSProp", "SGD"):
        cfg.optimizer = name
        net = make_net(8)
        opt = O.get_optimizer(cfg, net.parameters())
        set_grads([], [net.parameters()], torch.Generator().manual_seed(71), 1.0)
        p0 = [p.detach().clone() for p in net.parameters()]
        with pytest.raises(BBDMHipError):
            opt.step()
        assert all(torch.equal(p, q) for p, q in zip(net.parameters(), p0)), name
