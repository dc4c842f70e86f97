"""Shared bodies of the per-request sampling-parameter tests (SamplingParams in bbdm_amd/sampler.py and the two *_requests_* bridge
entry points of csrc/bridge.hip): run on the emulated kernels by tests/test_sampler_params_emu_cpu.py and on the GPU by
tests/test_sampler_params_gpu.py -- TEST INFRASTRUCTURE.

Kernel level: torch.equal throughout (the new kernels are instantiations of the existing ones' templates, under the same
-ffp-contract=off).  Sampler level: bitwise where both sides run the same kernels on the same batch (lockstep, defaults), LOOP_TOL of
tests/sampler_cases.py against the oracle's loop otherwise."""
import dataclasses

import pytest
import torch

import philox_cases as P
import sampler_cases as S
from fixtures import load_case, oracle_model, parity_err

IDLE, LAST, CLIP = 2, 1, 4


def _tables(dev):
    from bbdm_amd import bridge_schedule
    tables, _ = bridge_schedule(1000, "linear", 1.0, True, "linear", 200)
    return (torch.tensor(tables["m_t"], dtype=torch.float32, device=dev),
            torch.tensor(tables["variance_t"], dtype=torch.float32, device=dev))


def _ptr(t):
    return None if t is None else t.data_ptr()


def requests_step(x, y, pred, noise, m_t, var_t, t, t_next, flag, eta, objective, x_next, x0, alias, n=None):
    """bbdm_bb_p_sample_step_requests_f32 -> its return code (no exception: the argument checks are tested through it)."""
    from bbdm_amd import _lib
    return _lib.load().bbdm_bb_p_sample_step_requests_f32(
        x.data_ptr(), y.data_ptr(), pred.data_ptr(), noise.data_ptr(), m_t.data_ptr(), var_t.data_ptr(), t.data_ptr(),
        t_next.data_ptr(), flag.data_ptr(), _ptr(eta), objective, x_next.data_ptr(), x0.data_ptr(), _ptr(alias),
        x.shape[0] if n is None else n, x[0].numel(), S._stream(x.device))


def requests_philox_step(x, y, pred, seed, ordinal, m_t, var_t, t, t_next, flag, eta, objective, x_next, x0, alias, n=None):
    from bbdm_amd import _lib
    return _lib.load().bbdm_bb_p_sample_step_requests_philox_f32(
        x.data_ptr(), y.data_ptr(), pred.data_ptr(), seed.data_ptr(), ordinal.data_ptr(), m_t.data_ptr(), var_t.data_ptr(),
        t.data_ptr(), t_next.data_ptr(), flag.data_ptr(), _ptr(eta), objective, x_next.data_ptr(), x0.data_ptr(), _ptr(alias),
        x.shape[0] if n is None else n, x[0].numel(), S._stream(x.device))


# six images: one last step (2), one idle slot (3, with the clip bit set: only bits 0-1 are the state), two at the same step (1, 5)
# with different eta and clip; every image its own eta, one of them 0
T = [999, 494, 0, 37, 205, 494]
T_NEXT = [994, 489, 0, 32, 200, 489]
STATE = [0, 0, LAST, IDLE, 0, 0]
ETA = [1.0, 0.0, 0.5, float("nan"), 0.25, 0.75]
CLIPS = [1, 0, 1, 1, 0, 1]
ACTIVE = [0, 1, 2, 4, 5]


def _setup(dev, shape, off, with_noise):
    """Inputs of the kernel-level cases; every tensor starts ``off`` floats past its allocation.  The idle slot's inputs (and its eta)
    are NaN: read, they would show."""
    g = torch.Generator().manual_seed(11)
    N = len(T)
    x, y, pred, noise = (torch.randn((N,) + shape, generator=g) for _ in range(4))
    for a in (x, y, pred, noise):
        a[3] = float("nan")
    noise[2] = float("nan")                     # the last step reads no noise
    x, y, pred, noise = (P._offset(a.to(dev), off) for a in (x, y, pred, noise))
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    flag = i64([s | (CLIP if c else 0) for s, c in zip(STATE, CLIPS)])
    eta = torch.tensor(ETA, dtype=torch.float32, device=dev)
    return x, y, pred, (noise if with_noise else None), i64(T), i64(T_NEXT), flag, eta


def _check_against_scalar(got, x, y, pred, noise, m_t, var_t, objective):
    """Every active image of (x_next, x0_recon, alias) against bbdm_bb_p_sample_step_f32 run on that image alone with its own
    (t, t_next, is_last, eta, clip); the idle slot's rows keep the sentinel."""
    xn, x0, alias = got
    for a in got:
        assert bool((a[3] == S.SENTINEL).all()), objective
    for n in ACTIVE:
        sl = slice(n, n + 1)
        last = STATE[n] == LAST
        rn, r0 = S.scalar_step(x[sl].contiguous(), y[sl].contiguous(), pred[sl].contiguous(), noise[sl].contiguous(), m_t, var_t,
                               T[n], T_NEXT[n], 1 if last else 0, ETA[n], CLIPS[n], objective)
        assert bool(torch.isfinite(rn).all()) and bool(torch.isfinite(r0).all())
        assert torch.equal(xn[sl], rn) and torch.equal(alias[sl], rn), (objective, n, float((xn[sl] - rn).abs().max()))
        assert torch.equal(x0[sl], r0), (objective, n)
        if CLIPS[n]:
            assert float(r0.abs().max()) <= 1.0
    # the two images at the same step differ in eta and clip: the parameters are per image, not per step
    assert float(x0[5].abs().max()) <= 1.0 < float(x0[1].abs().max())


def kernel_per_image_params(dev):
    """1. N = 6 images of (3, 16, 20) at mixed steps, eta and clip per image: bit-equal to the scalar kernel, all three objectives."""
    m_t, var_t = _tables(dev)
    x, y, pred, noise, t, t_next, flag, eta = _setup(dev, (3, 16, 20), 0, True)
    for objective in (0, 1, 2):
        got = [torch.full_like(x, S.SENTINEL) for _ in range(3)]
        assert requests_step(x, y, pred, noise, m_t, var_t, t, t_next, flag, eta, objective, *got) == 0
        _check_against_scalar(got, x, y, pred, noise, m_t, var_t, objective)


SEED = [5, 2 ** 33 + 1, 77, 88, -9, 5]
ORDINAL = [0, 101, 199, 7, 2 ** 32 + 3, 101]


def kernel_per_image_params_philox(dev, shape, off):
    """2. The same for the Philox entry point against the fill kernel's tensor fed to the scalar kernel.  ``off`` = 1: pointers offset
    by 4 bytes (element path); shape (3, 5, 7): per_sample % 4 != 0 (element path with a ragged last group)."""
    from bbdm_amd import philox_normal
    m_t, var_t = _tables(dev)
    x, y, pred, _, t, t_next, flag, eta = _setup(dev, shape, off, False)
    seed, ordinal = (torch.tensor(v, dtype=torch.int64, device=dev) for v in (SEED, ORDINAL))
    noise = philox_normal(shape, seed, ordinal, domain=0)
    per_sample = x[0].numel()
    assert (per_sample % 4 == 0 and x.data_ptr() % 16 == 0) == (off == 0 and per_sample % 4 == 0)
    for objective in (0, 1, 2):
        got = [P._offset(torch.full_like(x, S.SENTINEL), off) for _ in range(3)]
        assert requests_philox_step(x, y, pred, seed, ordinal, m_t, var_t, t, t_next, flag, eta, objective, *got) == 0
        _check_against_scalar(got, x, y, pred, noise, m_t, var_t, objective)


def kernel_uniform_params(dev):
    """3. One eta and one clip for all images: torch.equal to bbdm_bb_p_sample_step_batched_f32 / _philox_f32."""
    from bbdm_amd import philox_normal
    m_t, var_t = _tables(dev)
    shape = (3, 16, 20)
    x, y, pred, noise, t, t_next, _, _ = _setup(dev, shape, 0, True)
    state = torch.tensor(STATE, dtype=torch.int64, device=dev)
    seed, ordinal = (torch.tensor(v, dtype=torch.int64, device=dev) for v in (SEED, ORDINAL))
    for objective in (0, 1, 2):
        for eta in (0.0, 0.5, 1.0):
            for clip in (0, 1):
                flag = state | (CLIP if clip else 0)
                etas = torch.full((len(T),), eta, dtype=torch.float32, device=dev)
                ref = [torch.full_like(x, S.SENTINEL) for _ in range(3)]
                S.batched_step(x, y, pred, noise, m_t, var_t, t, t_next, state, eta, clip, objective, *ref)
                got = [torch.full_like(x, S.SENTINEL) for _ in range(3)]
                assert requests_step(x, y, pred, noise, m_t, var_t, t, t_next, flag, etas, objective, *got) == 0
                ref_p = [torch.full_like(x, S.SENTINEL) for _ in range(3)]
                P._philox_step(x, y, pred, seed, ordinal, m_t, var_t, t, t_next, state, eta, clip, objective, *ref_p)
                got_p = [torch.full_like(x, S.SENTINEL) for _ in range(3)]
                assert requests_philox_step(x, y, pred, seed, ordinal, m_t, var_t, t, t_next, flag, etas, objective, *got_p) == 0
                for a, b, c, d in zip(got, ref, got_p, ref_p):
                    assert bool(torch.isfinite(b[ACTIVE]).all()) and bool((b[3] == S.SENTINEL).all())
                    assert torch.equal(a, b), (objective, eta, clip)
                    assert torch.equal(c, d), (objective, eta, clip)


def kernel_argument_checks(dev):
    """4. A null eta and N = 0 return a negative code and set bbdm_last_error(); nothing is launched (the outputs keep the sentinel)."""
    from bbdm_amd import _lib
    m_t, var_t = _tables(dev)
    x, y, pred, noise, t, t_next, flag, eta = _setup(dev, (3, 5, 7), 0, True)
    seed, ordinal = (torch.tensor(v, dtype=torch.int64, device=dev) for v in (SEED, ORDINAL))
    got = [torch.full_like(x, S.SENTINEL) for _ in range(3)]
    for name, rc in (
        ("requests: null eta", requests_step(x, y, pred, noise, m_t, var_t, t, t_next, flag, None, 0, *got)),
        ("requests: N = 0", requests_step(x, y, pred, noise, m_t, var_t, t, t_next, flag, eta, 0, *got, n=0)),
        ("requests_philox: null eta", requests_philox_step(x, y, pred, seed, ordinal, m_t, var_t, t, t_next, flag, None, 0, *got)),
        ("requests_philox: N = 0", requests_philox_step(x, y, pred, seed, ordinal, m_t, var_t, t, t_next, flag, eta, 0, *got, n=0)),
    ):
        assert rc < 0, name
        msg = _lib.load().bbdm_last_error()
        assert msg and b"p_sample_step_requests" in msg, (name, msg)
    torch.cuda.synchronize()
    for a in got:
        assert bool((a == S.SENTINEL).all())


# --------------------------------------------------------------------------------------------------------------
def tiny(dev, hip_graph=None, **bb):
    """tiny_concat (16 x 16 pixel BBDM) with ``bb`` over its bb_params -> (model, the record with those params)."""
    import bbdm_amd
    rec = load_case("tiny_concat")
    rec = dict(rec, bb_params=dict(rec["bb_params"], **bb))
    m = bbdm_amd.BrownianBridgeModel(S._ns({"BB": {"params": dict(rec["bb_params"], UNetParams=rec["unet_params"])}}))
    m.load_state_dict(rec["state_dict"], strict=True)
    m = m.to(dev).eval()
    if hip_graph is not None:
        m.denoise_fn.hip_graph = hip_graph
    return m, rec


def oracle_for(rec, params, clip_default):
    """The oracle configured with a request's params (None fields: the record's) -> (oracle, clip)."""
    bb = dict(rec["bb_params"])
    for k in ("sample_step", "skip_sample", "sample_type", "eta"):
        if getattr(params, k) is not None:
            bb[k] = getattr(params, k)
    ora = oracle_model(dict(rec, bb_params=bb))
    if params.steps is not None:
        ora.steps = torch.tensor(list(params.steps))           # the step table is a plain attribute, in the reference too
    return ora, clip_default if params.clip_denoised is None else params.clip_denoised


def _conds(n, dev, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 16, 16, generator=g).clamp(-1, 1).to(dev)


def lockstep_uniform_params(dev, hip_graph=None):
    """5. Model at sample_step 10 / eta 1; four requests with SamplingParams(sample_step=6, eta=0.5, clip_denoised=True) in a width-4
    Philox sampler == model6.sample(conds, clip_denoised=True, seeds=...), model6 the same weights at sample_step 6 / eta 0.5."""
    from bbdm_amd import BridgeSampler, SamplingParams
    m, _ = tiny(dev, hip_graph, sample_step=10, eta=1.0)
    m6, _ = tiny(dev, hip_graph, sample_step=6, eta=0.5)
    conds, seeds = _conds(4, dev, 3), [71, 72, 2 ** 40 + 73, 74]
    p = SamplingParams(sample_step=6, eta=0.5, clip_denoised=True)
    s = BridgeSampler(m, 4, clip_denoised=False, noise="philox")
    s.submit([(k, conds[k], seeds[k], p) for k in range(4)])
    got, steps = {}, 0
    while s.busy():
        got.update(s.step())
        steps += 1
    assert steps == 6 == len(m6.steps) and sorted(got) == [0, 1, 2, 3]
    ref = m6.sample(conds, clip_denoised=True, seeds=seeds)
    torch.cuda.synchronize()
    out = torch.stack([got[k] for k in range(4)])
    assert torch.equal(out, ref), float((out - ref).abs().max())


def simulate(width, lengths, groups, steps_between):
    """Host-only greedy simulation of the slot table: requests (their step-table lengths) arrive in ``groups`` with ``steps_between``
    sampler steps after each group but the last; a free slot takes the next queued request at the start of a step -> (number of
    steps, {request: the step it finishes in})."""
    queue, slots, finished, n = [], [None] * width, {}, 0

    def step():
        nonlocal n
        for j in range(width):
            if slots[j] is None and queue:
                slots[j] = [queue.pop(0), 0]
        n += 1
        for j in range(width):
            if slots[j] is not None:
                slots[j][1] += 1
                if slots[j][1] == lengths[slots[j][0]]:
                    finished[slots[j][0]] = n
                    slots[j] = None

    for gi, grp in enumerate(groups):
        queue += list(grp)
        if gi < len(groups) - 1:
            for _ in range(steps_between):
                step()
    while queue or any(s is not None for s in slots):
        step()
    return n, finished


def mixed_schedules(dev, noise, hip_graph=None):
    """6. Seven requests in a width-3 sampler (model: sample_step 10, eta 1): sample_step cycles over {4, 6, 10}, eta over {0, 0.5, 1},
    clip alternates, request 3 runs steps=[999, 500, 1, 0]; two groups, two steps apart.  Every key once, every result within
    LOOP_TOL of the oracle's loop for a model configured with the request's params, and the steps (in all and per request) are those
    of the greedy simulation of the slot table: short requests free their slots early."""
    from bbdm_amd import BridgeSampler, SamplingParams
    width, n_req = 3, 7
    m, rec = tiny(dev, hip_graph, sample_step=10, eta=1.0)
    conds = _conds(n_req, dev)
    seeds = [1000 + 7 * k for k in range(n_req - 1)] + [2 ** 40 + 3]
    params = []
    for k in range(n_req):
        kw = dict(eta=(0.0, 0.5, 1.0)[(k + k // 3) % 3], clip_denoised=k % 2 == 0)
        kw.update(dict(steps=[999, 500, 1, 0]) if k == 3 else dict(sample_step=(4, 6, 10)[k % 3]))
        params.append(SamplingParams(**kw))
    philox = noise == "philox"

    def gen(k):
        if philox:
            return seeds[k]
        g = torch.Generator(device=dev)
        g.manual_seed(seeds[k])
        return g

    s = BridgeSampler(m, width, clip_denoised=False, noise=noise)
    groups = [range(0, 4), range(4, n_req)]
    results, finished, steps = {}, {}, 0

    def step():
        nonlocal steps
        steps += 1
        for key, img in s.step():
            assert key not in results
            results[key], finished[key] = img, steps

    s.submit([(k, conds[k], gen(k), params[k]) for k in groups[0]])
    step()
    step()
    s.submit([(k, conds[k], gen(k), params[k]) for k in groups[1]])
    while s.busy():
        step()
    assert sorted(results) == list(range(n_req))
    oracles = [oracle_for(rec, params[k], False) for k in range(n_req)]
    lengths = [len(ora.steps) for ora, _ in oracles]
    assert lengths == [4, 6, 10, 4, 6, 10, 4]
    want_steps, want_finished = simulate(width, lengths, groups, 2)
    assert (steps, finished) == (want_steps, want_finished), (steps, finished, want_steps, want_finished)
    assert finished[0] < finished[3] < finished[2]              # request 3 ran in the slot request 0 freed while request 2 was mid-flight
    errs = {}
    for k in range(n_req):
        ora, clip = oracles[k]
        loop = P.philox_oracle_loop if philox else S.oracle_loop
        errs[k] = parity_err(results[k].cpu(), loop(ora, conds[k], clip, seeds[k], dev))
    print(f"mixed schedules ({noise}) vs oracle loop, per request:", {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(e < S.LOOP_TOL for e in errs.values()), errs


def defaults_and_sample_set(dev, hip_graph=None):
    """7. A four-tuple with SamplingParams() == the three-tuple, bitwise (same sampler, seeds, Philox noise).
    8. sample_set(..., params=SamplingParams(sample_step=4)) on a sampler whose model has sample_step 6: [M, sample_num, C, H, W], each
    sample within LOOP_TOL of the oracle at sample_step 4."""
    from bbdm_amd import BridgeSampler, SamplingParams
    m, rec = tiny(dev, hip_graph, sample_step=6)
    conds, seeds = _conds(2, dev, 5), [31, 2 ** 35 + 32, 33, 34]
    s = BridgeSampler(m, 2, clip_denoised=True, noise="philox")
    s.submit([(k, conds[k], seeds[k]) for k in range(2)])
    three = dict(s)
    s.submit([(k, conds[k], seeds[k], SamplingParams()) for k in range(2)])
    four = dict(s)
    s.submit([(0, conds[0], seeds[0], None), (1, conds[1], seeds[1])])
    none = dict(s)
    for k in range(2):
        assert torch.equal(three[k], four[k]) and torch.equal(three[k], none[k]), k

    p = SamplingParams(sample_step=4)
    out = s.sample_set(conds, 2, seeds, group=8, params=p)
    assert tuple(out.shape) == (2, 2, 3, 16, 16)
    ora, clip = oracle_for(rec, p, True)
    assert len(ora.steps) == 4
    for mi in range(2):
        for si in range(2):
            ref = P.philox_oracle_loop(ora, conds[mi], clip, seeds[mi * 2 + si], dev)
            err = parity_err(out[mi, si].cpu(), ref)
            print(f"sample_set(params=sample_step 4) sample ({mi}, {si}): {err:.2e}")
            assert err < S.LOOP_TOL, (mi, si, err)


def rejection(dev):
    """9. Every error of SamplingParams is raised at submit, before anything is queued -- also for a group whose first request is
    valid."""
    from bbdm_amd import BridgeSampler, SamplingParams
    m, _ = tiny(dev, sample_step=6)
    c = torch.zeros(3, 16, 16, device=dev)
    cases = [
        (IndexError, dict(sample_type="cosine")),                               # its table starts at t = num_timesteps
        (IndexError, dict(steps=[1000, 500, 0])),
        (ValueError, dict(sample_step=2)),                                       # (T - 1) / (sample_step - 2)
        (ValueError, dict(sample_step=2, skip_sample=True, sample_type="linear")),
        (ValueError, dict(steps=[500, 500, 0])),                                 # not strictly descending
        (ValueError, dict(steps=[100, 500, 0])),
        (ValueError, dict(steps=[999, 500, 1])),                                 # does not end in 0
        (ValueError, dict(steps=[999, 0, 0])),                                   # 0 elsewhere
        (ValueError, dict(steps=[])),
        (ValueError, dict(eta=-0.5)),
        (ValueError, dict(eta=float("inf"))),
        (ValueError, dict(eta=float("nan"))),
        (ValueError, dict(eta="1")),
        (NotImplementedError, dict(sample_type="quadratic")),
    ]
    for noise, good in (("torch", None), ("philox", 7)):
        s = BridgeSampler(m, 2, noise=noise)
        for exc, kw in cases:
            with pytest.raises(exc):
                s.submit([(0, c, good, SamplingParams(**kw))])
            assert not s.busy() and len(s._queue) == 0, kw
            with pytest.raises(exc):
                s.submit([(0, c, good, SamplingParams(sample_step=4)), (1, c, good, SamplingParams(**kw))])
            assert not s.busy() and len(s._queue) == 0, kw
        with pytest.raises(TypeError):
            s.submit([(0, c, good, dict(sample_step=4))])
        with pytest.raises(ValueError):
            s.submit([(0, c, good, None, None)])
        assert not s.busy() and len(s._queue) == 0
    # valid ones queue: skip_sample False ignores sample_type, as the reference does
    s = BridgeSampler(m, 2)
    s.submit([(0, c, None, SamplingParams(skip_sample=False, sample_type="quadratic")), (1, c, None, SamplingParams(eta=0))])
    assert len(s._queue) == 2 and len(s._queue[0].steps) == 1000 and s._queue[1].eta == 0.0
    with pytest.raises(dataclasses.FrozenInstanceError):
        SamplingParams().eta = 1.0
