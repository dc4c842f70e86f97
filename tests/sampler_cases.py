"""Shared bodies of the BridgeSampler tests (bbdm_amd/sampler.py): run on the emulated kernels by tests/test_sampler_emu_cpu.py and on
the GPU by tests/test_sampler_gpu.py -- TEST INFRASTRUCTURE."""
import argparse

import torch

import bbdm_oracle as O
from fixtures import load_case, oracle_model, parity_err

SENTINEL = 12345.0
LOOP_TOL = 5e-3        # tests/test_loop_parity_gpu.py:104, the free-running bar of a 200-step loop (these loops have 6 / 10 steps)


def _ns(c):
    ns = argparse.Namespace()
    for k, v in c.items():
        setattr(ns, k, _ns(v) if isinstance(v, dict) else v)
    return ns


def _stream(dev):
    from bbdm_amd import _lib
    return _lib.current_stream(dev)


def scalar_step(x, y, pred, noise, m_t, var_t, t, t_next, is_last, eta, clip, objective):
    """bbdm_bb_p_sample_step_f32 on a batch (all at one step) -> (x_next, x0_recon)."""
    from bbdm_amd import _lib
    xn, x0 = torch.empty_like(x), torch.empty_like(x)
    _lib.call("bbdm_bb_p_sample_step_f32", x.data_ptr(), y.data_ptr(), pred.data_ptr(), None if is_last else noise.data_ptr(),
              m_t.data_ptr(), var_t.data_ptr(), t, t_next, is_last, eta, clip, objective, xn.data_ptr(), x0.data_ptr(), None,
              x.shape[0], x[0].numel(), _stream(x.device))
    return xn, x0


def batched_step(x, y, pred, noise, m_t, var_t, t, t_next, flag, eta, clip, objective, x_next, x0, alias):
    from bbdm_amd import _lib
    _lib.call("bbdm_bb_p_sample_step_batched_f32", x.data_ptr(), y.data_ptr(), pred.data_ptr(), noise.data_ptr(), m_t.data_ptr(),
              var_t.data_ptr(), t.data_ptr(), t_next.data_ptr(), flag.data_ptr(), eta, clip, objective, x_next.data_ptr(),
              x0.data_ptr(), None if alias is None else alias.data_ptr(), x.shape[0], x[0].numel(), _stream(x.device))


def kernel_equivalence(dev):
    """N = 5 images at mixed steps (one last step, one inactive slot): every active image bit-equal to the scalar kernel run on that
    image alone with its own (t, t_next, is_last); the inactive slot's rows of x_next, x0_recon and the alias keep their sentinel."""
    from bbdm_amd import bridge_schedule
    tables, _ = bridge_schedule(1000, "linear", 1.0, True, "linear", 200)
    m_t = torch.tensor(tables["m_t"], dtype=torch.float32, device=dev)
    var_t = torch.tensor(tables["variance_t"], dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(11)
    N, shape = 5, (3, 16, 20)                   # per_sample 960: several blocks per image
    x, y, pred, noise = (torch.randn((N,) + shape, generator=g) for _ in range(4))
    t = torch.tensor([999, 494, 0, 37, 205], dtype=torch.int64)
    t_next = torch.tensor([994, 489, 0, 32, 200], dtype=torch.int64)
    flag = torch.tensor([0, 0, 1, 2, 0], dtype=torch.int64)
    for a in (x, y, pred, noise):
        a[3] = float("nan")                     # the inactive slot's inputs: read, they would show
    noise[2] = float("nan")                     # the last step reads no noise
    x, y, pred, noise, t, t_next, flag = (a.to(dev) for a in (x, y, pred, noise, t, t_next, flag))
    checked = 0
    for objective in (0, 1, 2):
        for eta in (0.0, 1.0):
            for clip in (0, 1):
                xn, x0, alias = (torch.full_like(x, SENTINEL) for _ in range(3))
                batched_step(x, y, pred, noise, m_t, var_t, t, t_next, flag, eta, clip, objective, xn, x0, alias)
                for n in range(N):
                    if int(flag[n]) == 2:
                        for a in (xn, x0, alias):
                            assert bool((a[n] == SENTINEL).all()), (objective, eta, clip)
                        continue
                    last = int(flag[n]) == 1
                    sl = slice(n, n + 1)
                    rn, r0 = scalar_step(x[sl].contiguous(), y[sl].contiguous(), pred[sl].contiguous(), noise[sl].contiguous(), m_t,
                                         var_t, int(t[n]), int(t_next[n]), 1 if last else 0, eta, clip, objective)
                    assert torch.equal(xn[sl], rn) and torch.equal(alias[sl], rn), (objective, eta, clip, n)
                    assert torch.equal(x0[sl], r0), (objective, eta, clip, n)
                    assert bool(torch.isfinite(rn).all())
                    checked += 1
    assert checked == 12 * 4


# --------------------------------------------------------------------------------------------------------------
def tiny_concat(dev, sample_step, hip_graph=None):
    """The golden tiny_concat case (pixel BBDM, condition_key SpatialRescaler: context = y) at ``sample_step`` -> (model, oracle)."""
    import bbdm_amd
    rec = load_case("tiny_concat")
    rec = dict(rec, bb_params=dict(rec["bb_params"], sample_step=sample_step))
    m = bbdm_amd.BrownianBridgeModel(_ns({"BB": {"params": dict(rec["bb_params"], UNetParams=rec["unet_params"])}}))
    m.load_state_dict(rec["state_dict"], strict=True)
    m = m.to(dev).eval()
    if hip_graph is not None:
        m.denoise_fn.hip_graph = hip_graph
    return m, oracle_model(rec)


def replay_noises(seed, shape, steps, dev):
    """The noise contract of BridgeSampler: per non-final step (steps[i] != 0) one torch.randn(shape) from a fresh generator on
    ``dev`` seeded with ``seed``, in step order; None at steps[i] == 0."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return [torch.randn(shape, generator=g, device=dev) if int(s) != 0 else None for s in steps]


def oracle_loop(ora, y, clip, seed, dev):
    """One image alone through the oracle's p_sample_loop with the request's replayed noise (CPU, fp32)."""
    noises = [None if e is None else e.cpu().unsqueeze(0) for e in replay_noises(seed, tuple(y.shape), ora.steps, dev)]
    return ora.p_sample_loop(y.cpu().unsqueeze(0), None, clip, noises=noises)[0]


def mixed_progress(dev, width, n_req, sample_step, clip=True, hip_graph=None):
    """``n_req`` requests through a ``width``-wide sampler, submitted in three groups at different steps: slots refill while other
    slots are mid-flight, and the tail runs with inactive slots.  Every request within LOOP_TOL of its own oracle loop; every key once."""
    from bbdm_amd import BridgeSampler
    m, ora = tiny_concat(dev, sample_step, hip_graph)
    g = torch.Generator().manual_seed(21)
    conds = torch.randn(n_req, 3, 16, 16, generator=g).clamp(-1, 1).to(dev)
    seeds = [1000 + 7 * k for k in range(n_req)]
    s = BridgeSampler(m, width, clip_denoised=clip)
    first = max(1, width - 1)                    # one slot idle at the start, filled by the second group mid-flight
    groups = [range(0, first), range(first, first + 1), range(first + 1, n_req)]
    results, stepped = {}, 0
    for gi, grp in enumerate(groups):
        reqs = []
        for k in grp:
            gen = torch.Generator(device=dev)
            gen.manual_seed(seeds[k])
            reqs.append((k, conds[k], gen))
        s.submit(reqs)
        for _ in range(2 if gi < 2 else 0):      # two steps before the next group arrives
            for key, img in s.step():
                assert key not in results
                results[key] = img
            stepped += 1
    for key, img in s:
        assert key not in results
        results[key] = img
    assert sorted(results) == list(range(n_req))
    errs = {}
    for k in range(n_req):
        ref = oracle_loop(ora, conds[k], clip, seeds[k], dev)
        errs[k] = parity_err(results[k].cpu(), ref)
    print("sampler vs oracle loop, per request:", {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(e < LOOP_TOL for e in errs.values()), errs
    return m, s, conds, seeds, ora


def sample_set_shape(dev, sampler, conds, seeds, ora, clip=True):
    """sample_set of two conditions x two samples: [M, sample_num, C, H, W], each sample within LOOP_TOL of its oracle loop."""
    out = sampler.sample_set(conds[:2], 2, seeds[:4], group=8)
    assert tuple(out.shape) == (2, 2, 3, 16, 16)
    for mi in range(2):
        for si in range(2):
            ref = oracle_loop(ora, conds[mi], clip, seeds[mi * 2 + si], dev)
            assert parity_err(out[mi, si].cpu(), ref) < LOOP_TOL, (mi, si)


def rejection(dev):
    """A condition of another shape raises RuntimeError (what the UNet call of p_sample raises); a 'cosine' schedule, which indexes the
    tables out of range (BrownianBridgeModel.py:74-77), raises IndexError at submission, as p_sample does."""
    import pytest
    from bbdm_amd import BridgeSampler
    m, _ = tiny_concat(dev, 6)
    s = BridgeSampler(m, 2)
    with pytest.raises(RuntimeError):
        s.submit([(0, torch.zeros(4, 16, 16, device=dev), None)])         # 4 + 4 channels into a 6-channel UNet
    s.submit([(0, torch.zeros(3, 16, 16, device=dev), None)])
    with pytest.raises(RuntimeError):
        s.submit([(1, torch.zeros(3, 8, 8, device=dev), None)])           # another resolution in the same sampler
    mc, _ = tiny_concat(dev, 6)
    mc.sample_type = "cosine"
    mc.register_schedule()
    with pytest.raises(IndexError):
        mc.p_sample(torch.zeros(1, 3, 16, 16, device=dev), torch.zeros(1, 3, 16, 16, device=dev),
                    torch.zeros(1, 3, 16, 16, device=dev), 0)
    sc = BridgeSampler(mc, 2)
    with pytest.raises(IndexError):
        sc.submit([(0, torch.zeros(3, 16, 16, device=dev), None)])
    assert not sc.busy()
