"""Kernel-level tests of the continuous latent plan's launches in csrc/losses.hip (hulc_gauss_plan_fwd / hulc_gauss_plan_bwd: reparameterised
Gaussian sample + KL-balanced diagonal-Gaussian KL) against float64 restatements built on torch.distributions.  The reference formulas are
hulc2/utils/distributions.py:28-29,55-59 (state), hulc2/models/hulc2.py:235-237 (rsample) and hulc2.py:444-466 (balanced KL with its two
detached copies).  The pattern of a case and the tolerance rule are in tests/kcheck.py."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch.distributions import Independent, Normal, kl_divergence

from tests import kcheck as K
from tests.kcheck import Guarded, compare, out_flat, refused, rnd, same_bits

pytestmark = pytest.mark.gpu

# Margins of margin * max(e_ref, 2^-23), e_ref = the float32 CPU evaluation of the same formula against float64 (tests/kcheck.py).
#   LIBM 4: the row of tests/test_losses_gpu.py — libm-accurate expf / logf / log1pf; against torch's float32 CPU code only the summation
#           order and fused multiply-adds differ.
# A case that cannot meet its margin is a finding and gets its own named row here with the measured errors and the cause.
MARGIN = {"LIBM": 4.0}

F32 = torch.float32
MIN_STD = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    K.report("tests/test_gauss_plan_gpu.py")


def _gen(*key):
    seed = 0
    for k in key:
        for ch in (k if isinstance(k, str) else repr(k)):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def _raw(g, B, P, family):
    """one head's raw output (B, 2P) = [mean | r], float64 of float32 values"""
    mean = _randn(g, B, P)
    if family == "tight":              # std on the min_std floor: softplus(-15) = 3e-7 beside 1e-4, 1 / std^2 = 1e8
        r = -15.0 + 0.5 * _randn(g, B, P)
    elif family == "wide":             # both sides of softplus's threshold 20
        r = 15.0 + 15.0 * _rand(g, B, P)
    else:
        r = _randn(g, B, P)
    return rnd(torch.cat([mean, r], 1), F32)


def _state(raw):
    mean, r = torch.chunk(raw, 2, dim=-1)
    return mean, F.softplus(r) + MIN_STD


def _dist(mean, std):
    return Independent(Normal(mean, std), 1)


def _kl_ref(pp, pr, beta, mix, gout, nseg, dt):
    """hulc2.py:444-466 per segment under torch autograd -> kl_row (B,), out (nseg,), dpp, dpr for the upstream gradient gout (nseg,)"""
    pp, pr = pp.to(dt).clone().requires_grad_(), pr.to(dt).clone().requires_grad_()
    (mp, sp), (mq, sq) = _state(pp), _state(pr)
    lhs = kl_divergence(_dist(mq.detach(), sq.detach()), _dist(mp, sp))        # gradient to the prior only
    rhs = kl_divergence(_dist(mq, sq), _dist(mp.detach(), sp.detach()))        # gradient to the posterior only
    out = beta * (mix * lhs.view(nseg, -1).mean(1) + (1.0 - mix) * rhs.view(nseg, -1).mean(1))
    (out * gout.to(dt)).sum().backward()
    return rhs.detach(), out.detach(), pp.grad, pr.grad


def _sample_ref(pr, eps, dplan, dt):
    """plan = mean + std * eps and its gradient w.r.t. the raw head output for the upstream dplan"""
    pr = pr.to(dt).clone().requires_grad_()
    mean, std = _state(pr)
    plan = mean + std * eps.to(dt)
    plan.backward(dplan.to(dt))
    return plan.detach(), pr.grad


SIZES = [(1, 1, 1), (2, 256, 2), (3, 7, 3), (64, 256, 2), (65, 256, 1), (1024, 256, 2)]     # (64, 256, 2): the benchmark's call
FAMILIES = ["normal", "tight", "wide", "equal"]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,P,nseg", SIZES)
def test_gauss_kl(dev, B, P, nseg, family):
    from hulc2_amd import kernels as kn

    g = _gen("gkl", B, P, nseg, family)
    beta, mix = 0.037, 0.8
    fam = "normal" if family == "equal" else family
    pp, pr = _raw(g, B, P, fam), _raw(g, B, P, fam)
    if family == "equal":
        pp = pr.clone()
    gout = rnd(0.5 + _rand(g, nseg), F32)                    # a different upstream gradient per segment
    d = lambda t: t.float().to(dev)
    out, klr = out_flat(dev, nseg), out_flat(dev, B)
    fwd = lambda: kn.gauss_plan_fwd(d(pp), d(pr), None, 0, B, P, beta, nseg, None, None, out.t, klr.t)
    fwd()
    torch.cuda.synchronize()
    out.assert_guards("out"); klr.assert_guards("kl_row")
    o1, k1 = out.value(), klr.value()
    dpp, dpr = Guarded(dev, B, 2 * P), Guarded(dev, B, 2 * P)
    bwd = lambda: kn.gauss_plan_bwd(d(pp), d(pr), None, 0, B, P, beta, mix, nseg, None, d(gout), dpp.t, dpr.t)
    bwd()
    torch.cuda.synchronize()
    dpp.assert_guards("dpp"); dpr.assert_guards("dpr")
    a1, b1 = dpp.value(), dpr.value()
    if family == "equal":
        assert (k1 == 0).all() and (o1 == 0).all() and (a1 == 0).all() and (b1 == 0).all(), "pp == pr: value and both gradients are exactly 0"
    else:
        r, f = _kl_ref(pp, pr, beta, mix, gout, nseg, torch.float64), _kl_ref(pp, pr, beta, mix, gout, nseg, F32)
        compare("gauss_plan_fwd", "kl_row", k1, r[0], f[0], MARGIN["LIBM"])
        compare("gauss_plan_fwd", "out", o1, r[1], f[1], MARGIN["LIBM"])
        compare("gauss_plan_bwd", "dpp", a1, r[2], f[2], MARGIN["LIBM"], grad=True)
        compare("gauss_plan_bwd", "dpr", b1, r[3], f[3], MARGIN["LIBM"], grad=True)
    dpp.t.fill_(float("nan")); dpr.t.fill_(float("nan")); out.t.fill_(float("nan")); klr.t.fill_(float("nan"))
    bwd(); fwd()
    torch.cuda.synchronize()
    same_bits(dpp.value(), a1, "gauss_plan_bwd dpp"); same_bits(dpr.value(), b1, "gauss_plan_bwd dpr")
    same_bits(out.value(), o1, "gauss_plan_fwd out"); same_bits(klr.value(), k1, "gauss_plan_fwd kl_row")


@pytest.mark.parametrize("family", ["normal", "tight", "wide"])
@pytest.mark.parametrize("B,P,nseg", SIZES)
def test_gauss_sample_with_injected_noise(dev, B, P, nseg, family):
    """plan = mean + std * eps with eps injected; eps_out returns the injected noise bit for bit; the backward for dplan alone, gout alone and
    both together (one launch: the sum of the two single calls)"""
    from hulc2_amd import kernels as kn

    g = _gen("gsample", B, P, nseg, family)
    beta, mix = 0.037, 0.8
    pp, pr = _raw(g, B, P, family), _raw(g, B, P, family)
    eps, dplan = rnd(_randn(g, B, P), F32), rnd(_randn(g, B, P), F32)
    gout = rnd(0.5 + _rand(g, nseg), F32)
    d = lambda t: t.float().to(dev)
    plan, eps_out = Guarded(dev, B, P), Guarded(dev, B, P)
    fwd = lambda: kn.gauss_plan_fwd(None, d(pr), d(eps), 7, B, P, 0.0, 1, plan.t, eps_out.t, None, None)
    fwd()
    torch.cuda.synchronize()
    plan.assert_guards("plan"); eps_out.assert_guards("eps_out")
    p1 = plan.value()
    r64, r32 = _sample_ref(pr, eps, dplan, torch.float64), _sample_ref(pr, eps, dplan, F32)
    compare("gauss_plan_fwd", "plan", p1, r64[0], r32[0], MARGIN["LIBM"])
    assert torch.equal(eps_out.value().cpu(), eps.float()), "eps_out is the injected noise, bit for bit"
    # all three parts in one forward call give the same plan bits and the KL of the KL-only call
    out, klr, plan2 = out_flat(dev, nseg), out_flat(dev, B), Guarded(dev, B, P)
    kn.gauss_plan_fwd(d(pp), d(pr), d(eps), 7, B, P, beta, nseg, plan2.t, None, out.t, klr.t)
    torch.cuda.synchronize()
    plan2.assert_guards("plan (with KL)"); out.assert_guards("out"); klr.assert_guards("kl_row")
    same_bits(plan2.value(), p1, "plan with and without the KL part")
    k64, k32 = _kl_ref(pp, pr, beta, mix, gout, nseg, torch.float64), _kl_ref(pp, pr, beta, mix, gout, nseg, F32)
    compare("gauss_plan_fwd", "out+sample", out.value(), k64[1], k32[1], MARGIN["LIBM"])

    def bwd(with_dplan, with_gout):
        dpp, dpr = Guarded(dev, B, 2 * P), Guarded(dev, B, 2 * P)
        kn.gauss_plan_bwd(d(pp) if with_gout else None, d(pr), d(eps), 7, B, P, beta, mix, nseg, d(dplan) if with_dplan else None,
                          d(gout) if with_gout else None, dpp.t if with_gout else None, dpr.t)
        torch.cuda.synchronize()
        dpp.assert_guards("dpp"); dpr.assert_guards("dpr")
        if not with_gout:
            dpp.assert_untouched("dpp without gout")
        return dpp.value(), dpr.value()

    _, s_only = bwd(True, False)
    compare("gauss_plan_bwd", "dpr(dplan)", s_only, r64[1], r32[1], MARGIN["LIBM"], grad=True)
    kp_only, k_only = bwd(False, True)
    compare("gauss_plan_bwd", "dpr(gout)", k_only, k64[3], k32[3], MARGIN["LIBM"], grad=True)
    both_pp, both = bwd(True, True)
    same_bits(both_pp, kp_only, "dpp with and without dplan")
    compare("gauss_plan_bwd", "dpr(both)", both, s_only.double() + k_only.double(), s_only + k_only, MARGIN["LIBM"], grad=True)
    compare("gauss_plan_bwd", "dpr(both)/ad", both, r64[1] + k64[3], r32[1] + k32[3], MARGIN["LIBM"], grad=True)
    same_bits(bwd(True, True)[1], both, "gauss_plan_bwd dpr")
    plan.t.fill_(float("nan"))
    fwd()
    torch.cuda.synchronize()
    same_bits(plan.value(), p1, "gauss_plan_fwd plan")


def test_gauss_device_noise(dev):
    """no eps_in: standard normal noise from the counter RNG.  N = 2^20 draws; every bound is a five-sigma statement of sampling theory for
    independent N(0, 1) values: the mean has standard deviation 1 / sqrt(N), the sample variance sqrt(2 / N), the lag-1 correlation
    1 / sqrt(N), the share beyond 3 is binomial with p = 2 (1 - Phi(3))."""
    from hulc2_amd import kernels as kn

    B, P = 4096, 256
    N = B * P
    assert N == 1 << 20
    r1 = math.log(math.expm1(1.0 - MIN_STD))                 # softplus(r1) + min_std = 1
    raw = torch.cat([torch.zeros(B, P), torch.full((B, P), r1)], 1).to(dev)
    words = kn.step_state(dev).clone()

    def draw(seed):
        plan, eps = Guarded(dev, B, P), Guarded(dev, B, P)
        kn.gauss_plan_fwd(None, raw, None, seed, B, P, 0.0, 1, plan.t, eps.t, None, None)
        torch.cuda.synchronize()
        plan.assert_guards("plan"); eps.assert_guards("eps_out")
        return plan.value(), eps.value()

    try:
        plan, eps = draw(0xA11CE)
        assert torch.isfinite(eps).all() and torch.isfinite(plan).all()
        e = eps.double().cpu().reshape(-1)
        std = (F.softplus(raw[:, P:].double().cpu()) + MIN_STD).reshape(-1)
        compare("gauss_plan_fwd", "plan(noise)", plan, std * e, (std.float() * e.float()), MARGIN["LIBM"])
        mean, var = e.mean().item(), e.var(unbiased=True).item()
        c = e - e.mean()
        lag1 = ((c[:-1] * c[1:]).sum() / (c * c).sum()).item()
        p3 = math.erfc(3.0 / math.sqrt(2.0))                 # P(|z| > 3) = 0.0026998
        share = (e.abs() > 3.0).double().mean().item()
        print(f"[noise] mean {mean:.3e} var-1 {var - 1:.3e} lag1 {lag1:.3e} share(|eps|>3) {share:.6f} (p {p3:.6f}) max|eps| {e.abs().max():.3f}")
        assert abs(mean) <= 5.0 / math.sqrt(N)
        assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / N)
        assert abs(lag1) <= 5.0 / math.sqrt(N)
        assert abs(share - p3) <= 5.0 * math.sqrt(p3 * (1.0 - p3) / N)
        same_bits(draw(0xA11CE)[1], eps, "the same seed and step word")
        assert not torch.equal(draw(0xB0B)[1], eps), "another seed must change the noise"
        kn.advance_step_state(dev, rng=True, step=False)
        assert not torch.equal(draw(0xA11CE)[1], eps), "another step word must change the noise"
    finally:
        kn.step_state(dev).copy_(words)
        torch.cuda.synchronize()


@pytest.mark.parametrize("B,P", [(3, 7), (64, 256)])
def test_gauss_backward_regenerates_the_noise(dev, B, P):
    """device noise is never stored: d r_pr / (dplan * sigmoid(r_pr)) of the backward is the eps_out of the forward"""
    from hulc2_amd import kernels as kn

    g = _gen("regen", B, P)
    pr = _raw(g, B, P, "normal")
    dplan = rnd(0.5 + _rand(g, B, P), F32)
    d = lambda t: t.float().to(dev)
    plan, eps, dpr = Guarded(dev, B, P), Guarded(dev, B, P), Guarded(dev, B, 2 * P)
    kn.gauss_plan_fwd(None, d(pr), None, 0xB0B, B, P, 0.0, 1, plan.t, eps.t, None, None)
    kn.gauss_plan_bwd(None, d(pr), None, 0xB0B, B, P, 0.0, 0.0, 1, d(dplan), None, None, dpr.t)
    torch.cuda.synchronize()
    plan.assert_guards("plan"); eps.assert_guards("eps_out"); dpr.assert_guards("dpr")
    e = eps.value().cpu()
    got = dpr.value().cpu()
    assert torch.equal(got[:, :P], dplan.float()), "d mean_pr = dplan"
    sig32 = torch.sigmoid(pr[:, P:].float())
    rec = got[:, P:].double() / (dplan * torch.sigmoid(pr[:, P:]))
    ref32 = (dplan.float() * e * sig32) / (dplan.float() * sig32)
    compare("gauss_plan_bwd", "eps(regen)", rec, e.double(), ref32, MARGIN["LIBM"])


def test_gauss_plan_refuses_what_it_cannot_run(dev):
    from hulc2_amd import kernels as kn

    B, P = 4, 6
    z = torch.zeros(B, 2 * P, device=dev)
    e = torch.zeros(B, P, device=dev)
    one = torch.ones(3, device=dev)
    plan, eps_out, out, klr = Guarded(dev, B, P), Guarded(dev, B, P), out_flat(dev, 3), out_flat(dev, B)
    dpp, dpr = Guarded(dev, B, 2 * P), Guarded(dev, B, 2 * P)
    outs = (plan, eps_out, out, klr)
    f = "hulc_gauss_plan_fwd: "
    refused(lambda: kn.gauss_plan_fwd(z, z, e, 0, B, P, 1.0, 1, None, None, None, klr.t), f + "nothing to compute (plan, eps_out and out are all null)", *outs)
    refused(lambda: kn.gauss_plan_fwd(z, None, e, 0, B, P, 1.0, 1, plan.t, eps_out.t, out.t, klr.t), f + "null pointer", *outs)
    refused(lambda: kn.gauss_plan_fwd(None, z, e, 0, B, P, 1.0, 1, plan.t, eps_out.t, out.t, klr.t), f + "null pointer", *outs)
    refused(lambda: kn.gauss_plan_fwd(z, z, e, 0, B, P, 1.0, 1, plan.t, eps_out.t, out.t, None), f + "null pointer", *outs)
    refused(lambda: kn.gauss_plan_fwd(z, z, e, 0, B, 0, 1.0, 1, plan.t, eps_out.t, out.t, klr.t), f + "needs B >= 1 and plan_features >= 1", *outs)
    refused(lambda: kn.gauss_plan_fwd(z, z, e, 0, 0, P, 1.0, 1, plan.t, eps_out.t, out.t, klr.t), f + "needs B >= 1 and plan_features >= 1", *outs)
    refused(lambda: kn.gauss_plan_fwd(z, z, e, 0, B, P, 1.0, 3, plan.t, eps_out.t, out.t, klr.t), f + "the batch must split evenly into nseg segments", *outs)
    refused(lambda: kn.gauss_plan_fwd(z, z, e, 0, B, P, 1.0, 0, plan.t, eps_out.t, out.t, klr.t), f + "the batch must split evenly into nseg segments", *outs)
    b = "hulc_gauss_plan_bwd: "
    refused(lambda: kn.gauss_plan_bwd(z, z, e, 0, B, P, 1.0, 0.8, 1, None, None, dpp.t, dpr.t), b + "nothing to compute (dplan and gout are both null)", dpp, dpr)
    refused(lambda: kn.gauss_plan_bwd(z, None, e, 0, B, P, 1.0, 0.8, 1, e, one, dpp.t, dpr.t), b + "null pointer", dpp, dpr)
    refused(lambda: kn.gauss_plan_bwd(z, z, e, 0, B, P, 1.0, 0.8, 1, e, one, dpp.t, None), b + "null pointer", dpp, dpr)
    refused(lambda: kn.gauss_plan_bwd(None, z, e, 0, B, P, 1.0, 0.8, 1, e, one, dpp.t, dpr.t), b + "null pointer", dpp, dpr)
    refused(lambda: kn.gauss_plan_bwd(z, z, e, 0, B, P, 1.0, 0.8, 1, e, one, None, dpr.t), b + "null pointer", dpp, dpr)
    refused(lambda: kn.gauss_plan_bwd(z, z, e, 0, B, 0, 1.0, 0.8, 1, e, one, dpp.t, dpr.t), b + "needs B >= 1 and plan_features >= 1", dpp, dpr)
    refused(lambda: kn.gauss_plan_bwd(z, z, e, 0, B, P, 1.0, 0.8, 3, e, one, dpp.t, dpr.t), b + "the batch must split evenly into nseg segments", dpp, dpr)
