"""Shared bodies of the seed-addressed-noise tests (bbdm_amd/csrc/philox.h, the three Philox kernels of bridge.hip, the ``seeds=``
keywords and ``BridgeSampler(noise="philox")``): run on the emulated kernels by tests/test_philox_emu_cpu.py and on the GPU by
tests/test_philox_gpu.py -- TEST INFRASTRUCTURE.

The oracle of the bit stream is ``philox4x32_10`` below: Philox4x32-10 written from the paper (Salmon, Moraes, Dror, Shaw, SC'11) in
NumPy uint64 arithmetic.  The library's words are read through the debug entry ``bbdm_philox_raw_u32`` (the device build of the same
inline function every kernel calls), not by inverting u(r): u(r) = ((r >> 8) + 0.5f) * 2^-24 is evaluated in fp32 and is exact only
for r >> 8 < 2^23 (above, the 25-bit sum rounds to even), so it cannot be inverted for every word.
The oracle of the normals evaluates the contract's formula in float64 from the oracle's own words, with u exact."""
import numpy as np
import pytest
import torch

import sampler_cases as S
from fixtures import load_case, parity_err

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

# Random123's known-answer vectors for philox4x32-10: (counter, key) -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (broadcastable), key: two -> the four uint32 output arrays.  Ten rounds; the key is bumped by the Weyl
    constants between rounds."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return [v.astype(np.uint32) for v in c]


def oracle_normals(per_sample, seed, ordinal, domain):
    """float64 evaluation of the noise contract for one image: key = seed (lo32, hi32), counter = (e / 4, ordinal lo32, ordinal hi32,
    domain), words (r0, r1) -> elements 4q, 4q+1 and (r2, r3) -> 4q+2, 4q+3 by Box-Muller on u(r) = ((r >> 8) + 0.5) 2^-24."""
    seed, ordinal = int(seed) & (2 ** 64 - 1), int(ordinal) & (2 ** 64 - 1)
    q = np.arange((per_sample + 3) // 4, dtype=np.uint64)
    r = philox4x32_10((q, ordinal & 0xFFFFFFFF, ordinal >> 32, domain), (seed & 0xFFFFFFFF, seed >> 32))
    u = [((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for w in r]
    z = np.empty((q.size, 4), dtype=np.float64)
    for h in (0, 1):
        R = np.sqrt(-2.0 * np.log(u[2 * h]))
        th = 2.0 * np.pi * u[2 * h + 1]
        z[:, 2 * h], z[:, 2 * h + 1] = R * np.cos(th), R * np.sin(th)
    return z.reshape(-1)[:per_sample]


def _stream(dev):
    from bbdm_amd import _lib
    return _lib.current_stream(dev)


def library_words(ctr_key, dev):
    """[n, 6] (c0 c1 c2 c3 k0 k1) -> [n, 4] uint32 through bbdm_philox_raw_u32."""
    from bbdm_amd import _lib
    ck = np.ascontiguousarray(np.asarray(ctr_key, dtype=np.uint32))
    src = torch.from_numpy(ck.view(np.int32)).to(dev)
    out = torch.zeros(ck.shape[0], 4, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        _lib.call("bbdm_philox_raw_u32", src.data_ptr(), out.data_ptr(), ck.shape[0], _stream(dev))
    return out.cpu().numpy().view(np.uint32)


# --------------------------------------------------------------------------------------------------------------
def bit_stream(dev):
    """1. Oracle and library reproduce the known-answer vectors; and agree on 4096 random (counter, key) pairs."""
    for ctr, key, want in KAT:
        got = [int(v) for v in philox4x32_10(ctr, key)]
        assert got == list(want), ("oracle", [hex(v) for v in got])
    lib = library_words([list(c) + list(k) for c, k, _ in KAT], dev)
    for row, (_, _, want) in zip(lib, KAT):
        assert [int(v) for v in row] == list(want), ("library", [hex(int(v)) for v in row])
    rng = np.random.default_rng(5)
    ck = rng.integers(0, 2 ** 32, size=(4096, 6), dtype=np.uint64).astype(np.uint32)
    ref = np.stack(philox4x32_10([ck[:, j] for j in range(4)], [ck[:, 4], ck[:, 5]]), axis=1)
    assert np.array_equal(library_words(ck, dev), ref)


SEEDS = [7, 2 ** 32 + 12345, 987654321]                # one >= 2^32
ORDINALS = [0, 2 ** 32 + 9, 5]                         # one >= 2^32
NORMAL_TOL = 1e-5      # theta rounded to fp32 near 2 pi (half an ulp = 2.4e-7) times R <= 5.9 is 1.4e-6; logf / sqrtf / sinf / cosf add a few ulp


def normals(dev):
    """2. philox_normal against the float64 evaluation of the formula, per_sample 960 and 961 (the tail), domains 0 and 1; different
    seed / ordinal / domain -> different values; same triple -> the same bits, in any slot."""
    from bbdm_amd import philox_normal
    worst = 0.0
    for per_sample in (960, 961):
        for domain in (0, 1):
            got = philox_normal((per_sample,), SEEDS, ORDINALS, domain=domain, device=dev)
            assert got.shape == (3, per_sample) and got.dtype == torch.float32
            for n in range(3):
                ref = oracle_normals(per_sample, SEEDS[n], ORDINALS[n], domain)
                err = float(np.abs(got[n].cpu().numpy().astype(np.float64) - ref).max())
                worst = max(worst, err)
                print(f"philox_normal per_sample={per_sample} domain={domain} image={n}: max abs err {err:.3e}")
                assert err <= NORMAL_TOL, (per_sample, domain, n, err)
    print(f"philox_normal worst abs err vs float64: {worst:.3e} (bound {NORMAL_TOL})")
    shape = (3, 16, 20)
    base = philox_normal(shape, SEEDS, ORDINALS, domain=0, device=dev)
    assert base.shape == (3,) + shape
    assert torch.equal(base.reshape(3, -1)[:, :960], philox_normal((960,), SEEDS, ORDINALS, device=dev))   # the shape is only a shape
    other_seed = philox_normal(shape, [SEEDS[0] + 1] + SEEDS[1:], ORDINALS, device=dev)
    other_ord = philox_normal(shape, SEEDS, [ORDINALS[0] + 1] + ORDINALS[1:], device=dev)
    other_dom = philox_normal(shape, SEEDS, ORDINALS, domain=1, device=dev)
    assert not torch.equal(other_seed[0], base[0]) and torch.equal(other_seed[1:], base[1:])
    assert not torch.equal(other_ord[0], base[0]) and torch.equal(other_ord[1:], base[1:])
    for n in range(3):
        assert not torch.equal(other_dom[n], base[n])
    hi = philox_normal(shape, [SEEDS[0] + 2 ** 32], [ORDINALS[0]], device=dev)           # the high words are part of key and counter
    assert not torch.equal(hi[0], base[0])
    hi = philox_normal(shape, [SEEDS[0]], [ORDINALS[0] + 2 ** 32], device=dev)
    assert not torch.equal(hi[0], base[0])
    assert torch.equal(philox_normal(shape, SEEDS, ORDINALS, device=dev), base)
    perm = [2, 0, 1]                                   # slot independence, bitwise; seeds / ordinals as int64 tensors this time
    sd = torch.tensor([SEEDS[p] for p in perm], dtype=torch.int64, device=dev)
    od = torch.tensor([ORDINALS[p] for p in perm], dtype=torch.int64, device=dev)
    moved = philox_normal(shape, sd, od)
    for slot, p in enumerate(perm):
        assert torch.equal(moved[slot], base[p])
    assert torch.equal(philox_normal(shape, [SEEDS[1]], 5, device=dev)[0],                  # one ordinal for all images
                       philox_normal(shape, [3, SEEDS[1]], [5, 5], device=dev)[1])


def distribution(dev):
    """3. 2^20 values: |mean| < 5 / sqrt(n), |var - 1| < 5 sqrt(2 / n) (five standard errors), all finite, max |z| <= 5.9."""
    from bbdm_amd import philox_normal
    n = 2 ** 20
    z = philox_normal((n // 4,), [11, 12, 13, 2 ** 40 + 14], [0, 1, 2, 3], device=dev).double().reshape(-1)
    assert z.numel() == n and bool(torch.isfinite(z).all())
    mean, var, top = float(z.mean()), float(z.var(unbiased=False)), float(z.abs().max())
    print(f"2^20 normals: mean {mean:+.3e} (bound {5 / n ** 0.5:.2e}), var - 1 {var - 1:+.3e} (bound {5 * (2 / n) ** 0.5:.2e}), max |z| {top:.3f}")
    assert abs(mean) < 5 / n ** 0.5
    assert abs(var - 1) < 5 * (2 / n) ** 0.5
    assert top <= 5.9


# --------------------------------------------------------------------------------------------------------------
def _offset(t, off):
    """A copy of ``t`` whose storage starts ``off`` floats (4 bytes each) past an allocation's start."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16 or off == 0
    return v


def _philox_step(x, y, pred, seed, ordinal, m_t, var_t, t, t_next, flag, eta, clip, objective, x_next, x0, alias):
    from bbdm_amd import _lib
    _lib.call("bbdm_bb_p_sample_step_philox_f32", x.data_ptr(), y.data_ptr(), pred.data_ptr(), seed.data_ptr(), ordinal.data_ptr(),
              m_t.data_ptr(), var_t.data_ptr(), t.data_ptr(), t_next.data_ptr(), flag.data_ptr(), eta, clip, objective,
              x_next.data_ptr(), x0.data_ptr(), alias.data_ptr(), x.shape[0], x[0].numel(), _stream(x.device))


def fused_step_equals_unfused(dev, shape, off):
    """4. The setup of sampler_cases.kernel_equivalence (5 images at mixed steps, one last step, one idle slot with NaN inputs and
    sentinel outputs, 3 objectives x eta {0, 1} x clip {0, 1}): the Philox step kernel equals the batched kernel fed philox_normal's
    tensor, torch.equal on x_next, x0_recon and the alias; the idle rows keep their sentinel.  ``off``: every tensor starts ``off``
    floats past its allocation (off = 1: pointers offset by 4 bytes)."""
    from bbdm_amd import bridge_schedule, philox_normal
    tables, _ = bridge_schedule(1000, "linear", 1.0, True, "linear", 200)
    m_t = torch.tensor(tables["m_t"], dtype=torch.float32, device=dev)
    var_t = torch.tensor(tables["variance_t"], dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(11)
    N = 5
    x, y, pred = (torch.randn((N,) + shape, generator=g) for _ in range(3))
    t = torch.tensor([999, 494, 0, 37, 205], dtype=torch.int64)
    t_next = torch.tensor([994, 489, 0, 32, 200], dtype=torch.int64)
    flag = torch.tensor([0, 0, 1, 2, 0], dtype=torch.int64)
    seed = torch.tensor([5, 2 ** 33 + 1, 77, 88, -9], dtype=torch.int64)
    ordinal = torch.tensor([0, 101, 199, 7, 2 ** 32 + 3], dtype=torch.int64)
    for a in (x, y, pred):
        a[3] = float("nan")                     # the inactive slot's inputs: read, they would show
    x, y, pred = (_offset(a.to(dev), off) for a in (x, y, pred))
    t, t_next, flag, seed, ordinal = (a.to(dev) for a in (t, t_next, flag, seed, ordinal))
    noise = philox_normal(shape, seed, ordinal, domain=0)
    assert bool(torch.isfinite(noise).all())
    per_sample = x[0].numel()
    assert (per_sample % 4 == 0 and x.data_ptr() % 16 == 0) == (off == 0 and per_sample % 4 == 0)
    checked = 0
    for objective in (0, 1, 2):
        for eta in (0.0, 1.0):
            for clip in (0, 1):
                ref = [torch.full_like(x, S.SENTINEL) for _ in range(3)]
                S.batched_step(x, y, pred, noise, m_t, var_t, t, t_next, flag, eta, clip, objective, *ref)
                got = [_offset(torch.full_like(x, S.SENTINEL), off) for _ in range(3)]
                _philox_step(x, y, pred, seed, ordinal, m_t, var_t, t, t_next, flag, eta, clip, objective, *got)
                for a, b, name in zip(got, ref, ("x_next", "x0_recon", "alias")):
                    assert bool((a[3] == S.SENTINEL).all()), (name, objective, eta, clip)
                    for n in (0, 1, 2, 4):
                        assert bool(torch.isfinite(b[n]).all())
                        assert torch.equal(a[n], b[n]), (name, objective, eta, clip, n, float((a[n] - b[n]).abs().max()))
                        checked += 1
                if eta == 1.0:                  # the noise is in the result at all: another seed moves x_next of the noisy images only
                    alt = [torch.full_like(x, S.SENTINEL) for _ in range(3)]
                    _philox_step(x, y, pred, seed + 1, ordinal, m_t, var_t, t, t_next, flag, eta, clip, objective, *alt)
                    assert not torch.equal(alt[0][0], got[0][0]) and torch.equal(alt[0][2], got[0][2])
                    assert torch.equal(alt[1][[0, 1, 2, 4]], got[1][[0, 1, 2, 4]])
    assert checked == 12 * 3 * 4


def step_formula(x, y, pred, z, m_t, var_t, t, t_next, last, eta, clip, objective):
    """One image's bridge step as torch fp32 tensor ops in the reference's order (BrownianBridgeModel.py:148-160, 186-201), on the
    CPU -> (x_next, x0_recon, S_next, S_0): S_* = the sum of the absolute values of the terms each result is formed from."""
    m, var = m_t[t], var_t[t]
    sig = torch.sqrt(var)
    if objective == 0:
        x0, s0 = x - pred, x.abs() + pred.abs()
    elif objective == 1:
        x0, s0 = (x - m * y - sig * pred) / (1.0 - m), (x.abs() + m * y.abs() + sig * pred.abs()) / (1.0 - m)
    else:
        x0, s0 = y - pred, y.abs() + pred.abs()
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    if last:
        return x0, x0, s0, s0
    m_nt, var_nt = m_t[t_next], var_t[t_next]
    sigma2 = (var - var_nt * (1.0 - m) ** 2 / (1.0 - m_nt) ** 2) * var_nt / var
    sigma_t = torch.sqrt(sigma2) * eta
    coef = torch.sqrt((var_nt - sigma2) / var)
    xn = (1.0 - m_nt) * x0 + m_nt * y + coef * (x - (1.0 - m) * x0 - m * y) + sigma_t * z
    sn = (1.0 - m_nt) * s0 + m_nt * y.abs() + coef * (x.abs() + (1.0 - m) * s0 + m * y.abs()) + sigma_t * z.abs()
    return xn, x0, sn, s0


def fused_step_follows_the_formula(dev):
    """The element route of the Philox step kernel with a ragged last group (N = 3, per_sample = 7: one group of four, one of three)
    against step_formula on philox_normal's tensor: a noisy step, a last step and an idle slot; 3 objectives x clip {0, 1}.

    Bound.  The kernel and step_formula evaluate the same sequence of IEEE fp32 operations (no contraction; HIP rounds sqrtf and the
    division correctly by default), so the results agree up to a last-place difference of a sqrt or a division where a library takes
    another route: two such operations feed x0_recon, five more feed x_next, each a relative 2^-23 of a term.  Hence
    |x0 - ref| <= 4 * 2^-23 * S_0 and |x_next - ref| <= 16 * 2^-23 * S_next elementwise (S_*: the sum of the terms' absolute values,
    the perturbation of x0 carried through its coefficients).  A wrong coefficient or a wrong element of the tail is not a
    last-place difference."""
    from bbdm_amd import bridge_schedule, philox_normal
    tables, _ = bridge_schedule(1000, "linear", 1.0, True, "linear", 200)
    m_c, var_c = (torch.tensor(tables[k], dtype=torch.float32) for k in ("m_t", "variance_t"))
    g = torch.Generator().manual_seed(17)
    N, shape = 3, (7,)
    x, y, pred = (torch.randn((N,) + shape, generator=g) for _ in range(3))
    t, t_next, flag = [494, 0, 37], [489, 0, 32], [0, 1, 2]
    seed = torch.tensor([5, 2 ** 33 + 1, 77], dtype=torch.int64, device=dev)
    ordinal = torch.tensor([0, 101, 7], dtype=torch.int64, device=dev)
    z = philox_normal(shape, seed, ordinal, domain=0).cpu()
    dx, dy, dp = (a.to(dev) for a in (x, y, pred))
    assert dx[0].numel() % 4 != 0
    dt, dn, df = (torch.tensor(v, dtype=torch.int64, device=dev) for v in (t, t_next, flag))
    eps = 2.0 ** -23
    for objective in (0, 1, 2):
        for clip in (0, 1):
            got = [torch.full_like(dx, S.SENTINEL) for _ in range(3)]
            _philox_step(dx, dy, dp, seed, ordinal, m_c.to(dev), var_c.to(dev), dt, dn, df, 1.0, clip, objective, *got)
            xn, x0, alias = (a.cpu() for a in got)
            assert torch.equal(xn, alias)
            assert bool((xn[2] == S.SENTINEL).all()) and bool((x0[2] == S.SENTINEL).all())
            for n in (0, 1):
                rn, r0, sn, s0 = step_formula(x[n], y[n], pred[n], z[n], m_c, var_c, t[n], t_next[n], flag[n] == 1, 1.0, clip, objective)
                e0, en = float(((x0[n] - r0).abs() / s0).max()), float(((xn[n] - rn).abs() / sn).max())
                print(f"objective {objective} clip {clip} image {n}: x0_recon {e0 / eps:.2f} x 2^-23 (bar 4), x_next {en / eps:.2f} x 2^-23 (bar 16)")
                assert e0 <= 4 * eps and en <= 16 * eps, (objective, clip, n, e0, en)


def fused_q_sample_equals_unfused(dev, shape, off):
    """4. (q_sample) bbdm_bb_q_sample_philox_f32 equals bbdm_bb_q_sample_f32 fed philox_normal(domain=1): x_t and target, all three
    objectives, bitwise."""
    from bbdm_amd import _lib, bridge_schedule, philox_normal
    tables, _ = bridge_schedule(1000, "linear", 1.0, True, "linear", 200)
    m_t = torch.tensor(tables["m_t"], dtype=torch.float32, device=dev)
    var_t = torch.tensor(tables["variance_t"], dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(12)
    N = 4
    x0, y = (_offset(torch.randn((N,) + shape, generator=g).to(dev), off) for _ in range(2))
    t = torch.tensor([0, 999, 412, 57], dtype=torch.int64, device=dev)
    seed = torch.tensor([1, 2 ** 35 + 2, -4, 3], dtype=torch.int64, device=dev)
    ordinal = torch.tensor([0, 2 ** 32 + 1, 17, 17], dtype=torch.int64, device=dev)
    noise = philox_normal(shape, seed, ordinal, domain=1)
    assert not torch.equal(noise, philox_normal(shape, seed, ordinal, domain=0))
    per_sample = x0[0].numel()
    for objective in (0, 1, 2):
        ref = [torch.full_like(x0, S.SENTINEL) for _ in range(2)]
        _lib.call("bbdm_bb_q_sample_f32", x0.data_ptr(), y.data_ptr(), noise.data_ptr(), t.data_ptr(), m_t.data_ptr(),
                  var_t.data_ptr(), ref[0].data_ptr(), ref[1].data_ptr(), N, per_sample, objective, _stream(dev))
        got = [_offset(torch.full_like(x0, S.SENTINEL), off) for _ in range(2)]
        _lib.call("bbdm_bb_q_sample_philox_f32", x0.data_ptr(), y.data_ptr(), seed.data_ptr(), ordinal.data_ptr(), t.data_ptr(),
                  m_t.data_ptr(), var_t.data_ptr(), got[0].data_ptr(), got[1].data_ptr(), N, per_sample, objective, _stream(dev))
        for a, b, name in zip(got, ref, ("x_t", "target")):
            assert bool(torch.isfinite(b).all())
            assert torch.equal(a, b), (name, objective, float((a - b).abs().max()))
        if objective == 1:
            assert torch.equal(got[1], noise)       # objective 'noise': the target is the generated value


# --------------------------------------------------------------------------------------------------------------
def philox_oracle_loop(ora, y, clip, seed, dev):
    """One image alone through the oracle's p_sample_loop fed philox_normal(shape, seed, i) as the noise of step i."""
    from bbdm_amd import philox_normal
    noises = [None if int(s) == 0 else philox_normal(tuple(y.shape), [seed], [i], device=dev).cpu()
              for i, s in enumerate(ora.steps)]
    return ora.p_sample_loop(y.cpu().unsqueeze(0), None, clip, noises=noises)[0]


def model_level(dev, hip_graph=None, extras=True):
    """5. tiny_concat, 6 steps, as sampler_cases.mixed_progress: 5 requests with int seeds through a width-3
    BridgeSampler(noise="philox") in three groups (refills mid-flight, idle tail); each within LOOP_TOL of the oracle's loop fed
    philox_normal(shape, seed, i); model.sample(y, seeds=s) likewise, and within 2 x LOOP_TOL of the sampler's result; sample_set
    passes its seeds through; the seed / generator type checks; p_losses(seeds=...) == p_losses(noise=philox_normal(domain=1)).
    ``extras``: two more model.sample runs (seeds as a tensor, sample_mid_step) -- minutes each on the emulator, so the GPU file only."""
    from bbdm_amd import BridgeSampler, philox_normal
    width, n_req, clip = 3, 5, True
    m, ora = S.tiny_concat(dev, 6, hip_graph)
    g = torch.Generator().manual_seed(21)
    conds = torch.randn(n_req, 3, 16, 16, generator=g).clamp(-1, 1).to(dev)
    seeds = [1000 + 7 * k for k in range(n_req - 1)] + [2 ** 40 + 3]
    s = BridgeSampler(m, width, clip_denoised=clip, noise="philox")
    first = width - 1                            # one slot idle at the start, filled by the second group mid-flight
    groups = [range(0, first), range(first, first + 1), range(first + 1, n_req)]
    results = {}
    for gi, grp in enumerate(groups):
        s.submit([(k, conds[k], seeds[k]) for k in grp])
        for _ in range(2 if gi < 2 else 0):      # two steps before the next group arrives
            for key, img in s.step():
                assert key not in results
                results[key] = img
    for key, img in s:
        assert key not in results
        results[key] = img
    assert sorted(results) == list(range(n_req))
    assert s._noise is None                      # no noise buffer in this mode
    refs = {k: philox_oracle_loop(ora, conds[k], clip, seeds[k], dev) for k in range(n_req)}
    errs = {k: parity_err(results[k].cpu(), refs[k]) for k in range(n_req)}
    print("philox sampler vs oracle loop, per request:", {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(e < S.LOOP_TOL for e in errs.values()), errs

    out = m.sample(conds, clip_denoised=clip, seeds=seeds)
    errs = {k: parity_err(out[k].cpu(), refs[k]) for k in range(n_req)}
    cross = {k: parity_err(out[k].cpu(), results[k].cpu()) for k in range(n_req)}
    print("model.sample(seeds=) vs oracle loop:", {k: f"{e:.2e}" for k, e in errs.items()})
    print("model.sample(seeds=) vs sampler:", {k: f"{e:.2e}" for k, e in cross.items()})
    assert all(e < S.LOOP_TOL for e in errs.values()), errs
    assert all(e < 2 * S.LOOP_TOL for e in cross.values()), cross
    if extras:
        again = m.sample(conds, clip_denoised=clip, seeds=torch.tensor(seeds, dtype=torch.int64, device=dev))
        assert torch.equal(again, out)           # a function of the seeds: nothing is drawn from any generator state
        mid, one_step = m.sample(conds, clip_denoised=clip, sample_mid_step=True, seeds=seeds)
        assert len(mid) == 7 and len(one_step) == 6 and torch.equal(mid[-1], out)

    ss = s.sample_set(conds[:2], 2, [seeds[0], seeds[4], seeds[1], 55], group=8)
    assert tuple(ss.shape) == (2, 2, 3, 16, 16)
    for (mi, si), k in {(0, 0): 0, (1, 0): 1}.items():      # (condition k, seed of request k) again: the request's result
        assert parity_err(ss[mi, si].cpu(), refs[k]) < S.LOOP_TOL

    with pytest.raises(TypeError):
        BridgeSampler(m, 2, noise="philox").submit([(0, conds[0], torch.Generator(device=dev))])
    with pytest.raises(TypeError):
        BridgeSampler(m, 2, noise="philox").submit([(0, conds[0], None)])
    with pytest.raises(TypeError):
        BridgeSampler(m, 2).submit([(0, conds[0], 1234)])
    with pytest.raises(ValueError):
        BridgeSampler(m, 2, noise="curand")

    rec = load_case("tiny_concat")
    x0, y, t = (rec[k].to(dev) for k in ("x0", "y", "t"))
    sd, od = [31 + k for k in range(x0.shape[0])], 4
    with torch.no_grad():
        l_seed, d_seed = m.p_losses(x0, y, y, t, seeds=sd, ordinals=od)
        noise = philox_normal(tuple(x0.shape[1:]), sd, od, domain=1, device=dev)
        l_noise, d_noise = m.p_losses(x0, y, y, t, noise=noise)
        l_zero, _ = m.p_losses(x0, y, y, t, seeds=sd)
        l_zero2, _ = m.p_losses(x0, y, y, t, noise=philox_normal(tuple(x0.shape[1:]), sd, 0, domain=1, device=dev))
    assert torch.equal(l_seed, l_noise) and torch.equal(d_seed["x0_recon"], d_noise["x0_recon"])
    assert torch.equal(l_zero, l_zero2) and not torch.equal(l_zero, l_seed)
    with pytest.raises(ValueError):
        m.p_losses(x0, y, y, t, noise=noise, seeds=sd)
    with pytest.raises(ValueError):
        m.q_sample(x0, y, t, ordinals=[0] * x0.shape[0])
