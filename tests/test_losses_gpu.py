"""Kernel-level tests of csrc/losses.hip (logistic-mixture NLL + gripper cross-entropy, balanced categorical KL, plan sampler, contrastive
loss, loss combiner, time-major actions) against float64 restatements of the reference formulas, at the shapes, layouts and segmentations
the launchers accept.  The pattern of a case and the tolerance rule are in tests/kcheck.py."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import kcheck as K
from tests.kcheck import Guarded, compare, out_flat, refused, rnd, same_bits

pytestmark = pytest.mark.gpu

# Margins of margin * max(e_ref, 2^-23), e_ref = the float32 CPU evaluation of the same formula against float64 (tests/kcheck.py).
#   LIBM 4: losses.hip uses libm-accurate expf / logf / log1pf / sinf / atan2f and says so of itself; against torch's float32 CPU code only
#           the summation order and fused multiply-adds differ.
# A case that cannot meet its margin is a finding: it gets its own row here with the measured float32-CPU and GPU errors and the cause.
# Rows raised from LIBM, with what was measured on an MI355X (GPU error / float32-CPU error, both against float64) and why.  One cause is
# behind all of them: the balanced KL and the contrastive loss form the log-sum-exp itself, lse = max + log(sum), and take x - lse from it,
# where torch's log-softmax takes (x - max) - log(sum).  The kernels' form rounds twice at the size of the largest logit (half a unit of
# 2^6 * 2^-23 each for logits in 64..128) and every probability exp(x - lse) carries that as a RELATIVE error; the CPU's form rounds at
# the size of x - max, O(1) for the classes that matter.  With logits of the model's own size (N(0, 1) for the KL, logit_scale 0.5) the
# same kernels stay below 2 x.  Taking the differences from the maximum first brings every row below 2 x, but moves the last bits of
# the training step's KL and contrastive gradients, so the kernels are left as they are and the rows say what their form costs.
#   KL_SPREAD 32: logits uniform over +-80.  cat_kl_fwd kl_group 3.578e-06 / 1.886e-07 = 19.0 x (test_cat_kl[3-32-3-spread]), 10.5 x
#           ([2-1-1-spread]); out 11.9 x; cat_kl_bwd dpp 2.216e-06 / 7.418e-08 = 18.6 x, dpr 2.679e-06 / 2.222e-07 = 12.1 x.
#   CLIP_CLAMP 32: logit_scale = ln 100, logits up to 100.  clip_loss_fwd loss 7.698e-05 / 3.917e-06 = 19.7 x, clip_loss_bwd dim
#           5.835e-05 / 6.430e-06 = 9.1 x, dtx 10.9 x (test_clip_loss[64-32-all-4.6..]): lse - L[r][r] and exp(L - lse) both cancel at
#           the size of the logits once the pairs are aligned, and the loss and the gradients are what is left.
#   CLIP_CLAMP_DSCALE 512: the same scale, clip_loss_bwd dscale 7.980e-04 / 1.960e-06 = 407 x ([64-32-all-4.6..]), 20.6 x
#           ([127-1-all-4.6..]), 17.8 x ([128-0-all-4.6..]).  dscale = sum dL * L: every row of dL should sum to 0, the rounding of lse
#           leaves it at eps * 64, and the product with the logits' common size (70..100 on the diagonal) turns that into the
#           result's error while the true terms cancel; 8e-4 of the logit_scale gradient in the aligned regime.
MARGIN = {"LIBM": 4.0, "KL_SPREAD": 32.0, "CLIP_CLAMP": 32.0, "CLIP_CLAMP_DSCALE": 512.0}

F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    K.report("tests/test_losses_gpu.py")


def _gen(*key):
    """a generator seeded from the case's own parameters (stable across processes: no str hash)"""
    seed = 0
    for k in key:
        for ch in (k if isinstance(k, str) else repr(k)):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------
# logistic mixture + gripper cross-entropy
# ------------------------------------------------------------------------------------------------
# n_mix, A, T, ld (0 = the minimum 3 * A * n_mix + 2), ld_dy (0 = minimum), nseg, time_major_B, asymmetric bounds, num_classes,
# gripper_alpha, log_scale_min, family
MIX = [
    (10, 6, 2048, 184, 184, 1, 0, False, 10, 1.0, -7.0, "model"),      # the benchmark's call: 64 x 32 tokens, padded head output
    (10, 6, 2112, 184, 256, 2, 64, True, 10, 1.0, -3.5, "model"),      # both modalities time-major (33 steps x 64 rows), dy in a wider tensor
    (10, 6, 65, 184, 184, 1, 5, False, 256, 0.0, -7.0, "model"),       # time-major with one segment; no gripper term; fine bins
    (10, 1, 2112, 256, 184, 4, 0, True, 10, 1.0, -3.5, "model"),       # four batch-major segments of 528 tokens; ld > ld_dy
    (16, 6, 64, 0, 0, 4, 0, True, 256, 0.0, -3.5, "wide"),             # the most components, minimum pitch (290), segments of 16 tokens
    (16, 1, 2048, 0, 256, 4, 16, False, 10, 1.0, -3.5, "wide"),        # time-major, 4 batch rows per segment
    (16, 6, 63, 0, 0, 1, 0, True, 10, 1.0, -7.0, "wide"),              # one token short of 64
    (5, 6, 64, 0, 184, 2, 4, True, 10, 1.0, -3.5, "narrow"),           # 11 of the 16 mixture lanes idle; time-major B = 4, nseg = 2
    (5, 1, 65, 256, 0, 1, 0, False, 256, 1.0, -3.5, "narrow"),         # one action dimension: every other item is a gripper item
    (1, 6, 63, 184, 0, 1, 0, True, 10, 1.0, -3.5, "narrow"),           # a single component: the mixture weight's gradient is exactly 0
    (1, 1, 1, 0, 0, 1, 0, False, 10, 1.0, -7.0, "narrow"),             # the smallest call: two items
    (5, 6, 2048, 184, 184, 2, 0, False, 10, 0.0, -3.5, "narrow"),
]


def _mix_inputs(case):
    """-> y (T, W) float64 of float32 values, act (T, A + 1), act_min, act_max (A,), branch populations.  No item sits on a threshold of the
    reference's torch.where ladder: actions are exactly a bound or at least 0.01 inside it, and a component whose float64 cdf_delta falls
    within 1e-6 of 1e-5 has its mean redrawn until it does not (float32 and float64 deltas differ by ~1e-7 there)."""
    n_mix, A, T, ld, ld_dy, nseg, tmB, asym, ncls, alpha, lsm, family = case
    g = _gen("mix", *case[:7])
    lo = torch.tensor([-1.0, -0.5, -2.0, -1.0, -0.25, -1.5][:A], dtype=torch.float64) if asym else -torch.ones(A, dtype=torch.float64)
    hi = torch.tensor([1.0, 0.75, 3.0, 0.5, 0.25, 1.0][:A], dtype=torch.float64) if asym else torch.ones(A, dtype=torch.float64)
    u = _rand(g, T, A)
    a = rnd(lo + 0.01 + (hi - lo - 0.02) * _rand(g, T, A), F32).clamp(lo + 0.01, hi - 0.01)
    a = torch.where(u < 0.15, lo.expand(T, A), torch.where(u > 0.85, hi.expand(T, A), a))
    a = rnd(a, F32)
    assert (((a == lo) | (a >= lo + 0.0099)) & ((a == hi) | (a <= hi - 0.0099))).all()
    grip = torch.where(_rand(g, T, 1) < 0.5, -1.0, 1.0).double()
    logit = rnd(_randn(g, T, A, n_mix), F32)
    ls = rnd(_rand(g, T, A, n_mix) * 6.0 - 5.0, F32)                  # log-scales uniform in [-5, 1]: both sides of log_scale_min = -3.5
    assert not (ls == lsm).any()
    mu = rnd(_randn(g, T, A, n_mix) * 0.7, F32)
    half = ((hi - lo) / 2.0 / (ncls - 1))[None, :, None]

    def delta(mu):
        inv = torch.exp(-ls.clamp(min=lsm))
        c = a[:, :, None] - mu
        return torch.sigmoid(inv * (c + half)) - torch.sigmoid(inv * (c - half))

    redrawn = 0
    for _ in range(200):
        near = (delta(mu) - 1e-5).abs() < 1e-6
        if not near.any():
            break
        redrawn += int(near.sum())
        mu = torch.where(near, rnd(_randn(g, T, A, n_mix) * 0.7, F32), mu)
    excluded = int(((delta(mu) - 1e-5).abs() < 1e-6).sum())
    d = delta(mu)
    at_lo, at_hi = (a == lo)[:, :, None].expand_as(d), (a == hi)[:, :, None].expand_as(d)
    mid = ~at_lo & ~at_hi
    pops = dict(lower=int(at_lo.sum()), upper=int(at_hi.sum()), bin=int((mid & (d > 1e-5)).sum()), tail=int((mid & (d <= 1e-5)).sum()),
                clamped=int((ls < lsm).sum()), excluded=excluded, redrawn=redrawn)
    y = torch.cat([logit.reshape(T, -1), mu.reshape(T, -1), ls.reshape(T, -1), rnd(_randn(g, T, 2), F32)], 1)
    return y, torch.cat([a, grip], 1), lo, hi, pops


def _mix_seg_of_row(T, nseg, tmB):
    t = torch.arange(T)
    return t // (T // nseg) if tmB == 0 else (t % tmB) // (tmB // nseg)


def _mix_ref(y, act, lo, hi, n_mix, ncls, lsm, alpha, seg_of_row, nseg):
    """LogisticDecoderRNN._logistic_loss (+ log_sum_exp) with per-dimension bounds, and the gripper cross-entropy of _loss, per segment:
    -> (3, nseg) = totals | NLL means | CE means.  Written in the reference's own order of operations, in the dtype of y."""
    T, A = act.shape[0], act.shape[1] - 1
    n = A * n_mix
    logit, means, log_scales = (y[:, i * n:(i + 1) * n].reshape(T, A, n_mix) for i in range(3))
    log_scales = torch.clamp(log_scales, min=lsm)
    a = act[:, :A, None] * torch.ones_like(means)
    lo_, hi_ = lo.to(y.dtype)[None, :, None], hi.to(y.dtype)[None, :, None]
    centered = a - means
    inv_stdv = torch.exp(-log_scales)
    half = (hi_ - lo_) / 2.0 / (ncls - 1)
    plus_in = inv_stdv * (centered + half)
    cdf_plus = torch.sigmoid(plus_in)
    min_in = inv_stdv * (centered - half)
    cdf_min = torch.sigmoid(min_in)
    log_cdf_plus = plus_in - F.softplus(plus_in)
    log_one_minus_cdf_min = -F.softplus(min_in)
    mid_in = inv_stdv * centered
    log_pdf_mid = mid_in - log_scales - 2.0 * F.softplus(mid_in)
    cdf_delta = cdf_plus - cdf_min
    log_probs = torch.where(a < lo_ + 1e-3, log_cdf_plus,
                            torch.where(a > hi_ - 1e-3, log_one_minus_cdf_min,
                                        torch.where(cdf_delta > 1e-5, torch.log(torch.clamp(cdf_delta, min=1e-12)),
                                                    log_pdf_mid - math.log((ncls - 1) / 2))))
    log_probs = log_probs + F.log_softmax(logit, dim=-1)
    m = log_probs.max(dim=-1).values
    lse = m + torch.log(torch.sum(torch.exp(log_probs - m.unsqueeze(-1)), dim=-1))
    nll_tok = -lse.sum(-1)
    label = torch.where(act[:, A] == -1, 0, 1).long()
    ce_tok = F.cross_entropy(y[:, 3 * n:3 * n + 2], label, reduction="none")
    onehot = F.one_hot(seg_of_row, nseg).to(y.dtype)
    nll, ce = (nll_tok @ onehot) / (T // nseg), (ce_tok @ onehot) / (T // nseg)
    return torch.stack([nll + alpha * ce, nll, ce])


def _mix_run(dev, case, through_fn=False):
    from hulc2_amd import functional as HF, kernels as kn

    n_mix, A, T, ld, ld_dy, nseg, tmB, asym, ncls, alpha, lsm, family = case
    W = 3 * A * n_mix + 2
    ld, ld_dy = ld or W, ld_dy or W
    y, act, lo, hi, pops = _mix_inputs(case)
    assert pops["excluded"] == 0, "an item sits on the cdf_delta threshold"
    seg = _mix_seg_of_row(T, nseg, tmB)
    ybuf = torch.full((T, ld), float("nan"), device=dev)             # the padding columns of the head output are never read
    ybuf[:, :W] = y.float().to(dev)
    actd, lod, hid = act.float().to(dev), lo.float().to(dev), hi.float().to(dev)
    cfg = (T, A, n_mix, ncls, ld, lsm, alpha, lod, hid)
    out = Guarded(dev, 3, nseg)
    kn.mix_loss_fwd(ybuf, actd, out.t, *cfg, nseg=nseg, time_major_B=tmB)
    torch.cuda.synchronize()
    out.assert_guards("out")
    o1 = out.value()

    def ref(dt):
        yy = y.detach().clone().to(dt).requires_grad_()
        r = _mix_ref(yy, act.to(dt), lo, hi, n_mix, ncls, lsm, alpha, seg, nseg)
        return yy, r

    gout = rnd(0.5 + _rand(_gen("gout", *case[:7]), nseg), F32)      # a different upstream gradient per segment
    (y64, r64), (y32, r32) = ref(torch.float64), ref(F32)
    for i, nm in enumerate(("total", "nll", "ce")):
        compare("mix_loss_fwd", nm, o1[i], r64[i].detach(), r32[i].detach(), MARGIN["LIBM"])
    out.t.fill_(float("nan"))
    kn.mix_loss_fwd(ybuf, actd, out.t, *cfg, nseg=nseg, time_major_B=tmB)
    torch.cuda.synchronize()
    same_bits(out.value(), o1, "mix_loss_fwd")

    dy = Guarded(dev, T, ld_dy)                                      # every column of the ld_dy-wide rows is written (pad columns as zeros)
    kn.mix_loss_bwd(ybuf, actd, gout.float().to(dev), dy.t, ld_dy, *cfg, nseg=nseg, time_major_B=tmB)
    torch.cuda.synchronize()
    dy.assert_guards("dy")
    d1 = dy.value()
    (r64[0] * gout).sum().backward()
    (r32[0] * gout.float()).sum().backward()
    compare("mix_loss_bwd", "dy", d1[:, :W], y64.grad, y32.grad, MARGIN["LIBM"], grad=True)
    assert (d1[:, W:] == 0).all(), "the pad columns past 3 * A * n_mix + 2 carry exact zeros"
    n = A * n_mix
    below = (y[:, 2 * n:3 * n] < lsm)
    assert (d1[:, 2 * n:3 * n].cpu()[below] == 0).all(), "a log-scale below log_scale_min has gradient exactly 0"
    if n_mix == 1:
        assert (d1[:, :n] == 0).all(), "a single component's mixture logit has gradient exactly 0"
    if alpha == 0.0:
        assert (d1[:, 3 * n:W] == 0).all()
    dy.t.fill_(float("nan"))
    kn.mix_loss_bwd(ybuf, actd, gout.float().to(dev), dy.t, ld_dy, *cfg, nseg=nseg, time_major_B=tmB)
    torch.cuda.synchronize()
    same_bits(dy.value(), d1, "mix_loss_bwd")

    if through_fn:                                                   # the autograd wrapper hands the same numbers on
        yp = ybuf.clone().requires_grad_()
        loss = HF.MixLossFn.apply(yp, actd, lod, hid, n_mix, ncls, lsm, alpha, nseg, tmB)
        assert torch.equal(loss.detach().reshape(-1), o1[0])
        (loss.reshape(-1) * gout.float().to(dev)).sum().backward()
        torch.cuda.synchronize()
        assert yp.grad.shape == ybuf.shape and torch.equal(yp.grad[:, :W], d1[:, :W]) and (yp.grad[:, W:] == 0).all()


@pytest.mark.parametrize("case", MIX, ids=lambda c: "-".join(str(v) for v in c[:7]))
def test_mix_loss(dev, case):
    _mix_run(dev, case, through_fn=case[2] in (2112, 64))


def test_mix_loss_cases_populate_every_branch():
    """per family of MIX: the lower-bound, upper-bound, bin (cdf_delta > 1e-5) and tail branches of the ladder and the clamped log-scales all
    occur, and no component was left on the cdf_delta threshold"""
    fam = {}
    for case in MIX:
        pops = _mix_inputs(case)[4]
        assert pops["excluded"] == 0
        f = fam.setdefault(case[-1], dict.fromkeys(pops, 0))
        for k, v in pops.items():
            f[k] += v
    for name, f in fam.items():
        print(f"[kcheck] mix family {name}: {f}")
        for k in ("lower", "upper", "bin", "tail", "clamped"):
            assert f[k] > 0, f"family {name}: no component takes the {k} branch"


def test_mix_loss_refuses_what_it_cannot_run(dev):
    from hulc2_amd import kernels as kn

    T, A = 8, 1
    lo, hi = -torch.ones(A, device=dev), torch.ones(A, device=dev)
    y, act = torch.zeros(T, 64, device=dev), torch.zeros(T, A + 1, device=dev)
    out, dy, g = Guarded(dev, 3, 4), Guarded(dev, T, 64), torch.ones(4, device=dev)
    for kw, msg in ((dict(n_mix=17, nseg=1), "hulc_mix_loss: n_mix must be in 1..16"),
                    (dict(n_mix=4, nseg=3), "hulc_mix_loss: T must split into nseg equal segments"),
                    (dict(n_mix=4, nseg=2, time_major_B=3), "hulc_mix_loss: time-major rows need T % B == 0 and B % nseg == 0")):
        nm = kw.pop("n_mix")
        refused(lambda: kn.mix_loss_fwd(y, act, out.t, T, A, nm, 10, 64, -7.0, 1.0, lo, hi, **kw), msg, out)
        refused(lambda: kn.mix_loss_bwd(y, act, g, dy.t, 64, T, A, nm, 10, 64, -7.0, 1.0, lo, hi, **kw), msg, dy)


# ------------------------------------------------------------------------------------------------
# balanced categorical KL
# ------------------------------------------------------------------------------------------------
# B, G, nseg, family
KL = [
    (1, 1, 1, "normal"),        # one group: 7 of the workgroup's 8 sub-waves leave at once
    (2, 32, 2, "normal"),       # one row per segment
    (3, 32, 3, "spread"),       # logits over +-80: exp underflows to 0 for most classes, p * (lp - lq) must stay finite
    (64, 32, 2, "normal"),      # the benchmark's call: both modalities of 32 rows
    (65, 32, 1, "onehot"),      # near-one-hot posteriors; 2080 groups: the sum kernel's stride loop takes three trips
    (64, 1, 1, "equal"),        # pp == pr: value and both gradients exactly 0
    (3, 1, 3, "equal"),
    (2, 1, 1, "spread"),
    (64, 32, 1, "onehot"),
    (65, 1, 1, "normal"),
]


def _kl_ref(pp, pr, G, beta, mix, gout, nseg):
    """Hulc2.compute_kl_loss with KL balancing: value = beta * mean_rows(sum_groups KL(post || prior)); the posterior side (1 - mix) and the
    prior side (mix) of the gradient come from the two detached copies"""
    B = pp.shape[0]
    lp, lq = F.log_softmax(pr.reshape(B, G, 32), -1), F.log_softmax(pp.reshape(B, G, 32), -1)
    p, q = lp.exp(), lq.exp()
    klg = (p * (lp - lq)).sum(-1)
    Bs = B // nseg
    out = beta * klg.reshape(nseg, Bs * G).sum(-1) / Bs
    s = (gout.to(pp.dtype) * beta / Bs).repeat_interleave(Bs)[:, None, None]
    dpp = s * mix * (q - p)
    dpr = s * (1.0 - mix) * p * (lp - lq - klg[..., None])
    return klg.reshape(-1), out, dpp.reshape(B, -1), dpr.reshape(B, -1)


@pytest.mark.parametrize("B,G,nseg,family", KL)
def test_cat_kl(dev, B, G, nseg, family):
    from hulc2_amd import kernels as kn

    g = _gen("kl", B, G, nseg, family)
    beta, mix = 0.037, 0.8
    pp, pr = _randn(g, B, G * 32), _randn(g, B, G * 32)
    if family == "spread":
        pp, pr = (_rand(g, B, G * 32) * 160 - 80), (_rand(g, B, G * 32) * 160 - 80)
    elif family == "onehot":
        hot = F.one_hot(torch.randint(0, 32, (B, G), generator=g), 32).double().reshape(B, G * 32)
        pr = 30.0 * hot + 0.1 * pr
    pp, pr = rnd(pp, F32), rnd(pr, F32)
    if family == "equal":
        pp = pr.clone()
    gout = rnd(0.5 + _rand(g, nseg), F32)
    d = lambda t: t.float().to(dev)
    out, klg = out_flat(dev, nseg), out_flat(dev, B * G)
    kn.cat_kl_fwd(d(pp), d(pr), B, G, 32, beta, out.t, klg.t, nseg)
    torch.cuda.synchronize()
    out.assert_guards("out"); klg.assert_guards("kl_group")
    o1, k1 = out.value(), klg.value()
    r, f = _kl_ref(pp, pr, G, beta, mix, gout, nseg), _kl_ref(pp.float(), pr.float(), G, beta, mix, gout, nseg)
    m_fwd = MARGIN["KL_SPREAD" if family == "spread" else "LIBM"]
    compare("cat_kl_fwd", "kl_group", k1, r[0], f[0], m_fwd)
    compare("cat_kl_fwd", "out", o1, r[1], f[1], m_fwd)
    klg32 = rnd(r[0], F32)                                           # the saved per-group values, float32-rounded reference
    dpp, dpr = Guarded(dev, B, G * 32), Guarded(dev, B, G * 32)
    args = (d(pp), d(pr), d(klg32), B, G, 32, beta, mix, d(gout), dpp.t, dpr.t, nseg)
    kn.cat_kl_bwd(*args)
    torch.cuda.synchronize()
    dpp.assert_guards("dpp"); dpr.assert_guards("dpr")
    a1, b1 = dpp.value(), dpr.value()
    if family == "equal":
        assert (k1 == 0).all() and (o1 == 0).all() and (a1 == 0).all() and (b1 == 0).all(), "pp == pr: value and both gradients are exactly 0"
    else:
        def bwd(dt):
            x = _kl_ref(pp.to(dt), pr.to(dt), G, beta, mix, gout, nseg)
            lp, lq = F.log_softmax(pr.to(dt).reshape(B, G, 32), -1), F.log_softmax(pp.to(dt).reshape(B, G, 32), -1)
            s = (gout.to(dt) * beta / (B // nseg)).repeat_interleave(B // nseg)[:, None, None]
            return x[2], (s * (1.0 - mix) * lp.exp() * (lp - lq - klg32.to(dt).reshape(B, G, 1))).reshape(B, -1)      # from the SAVED kl_group

        rb, fb = bwd(torch.float64), bwd(F32)
        compare("cat_kl_bwd", "dpp", a1, rb[0], fb[0], m_fwd, grad=True)
        compare("cat_kl_bwd", "dpr", b1, rb[1], fb[1], m_fwd, grad=True)
    dpp.t.fill_(float("nan")); dpr.t.fill_(float("nan")); out.t.fill_(float("nan"))
    kn.cat_kl_bwd(*args)
    kn.cat_kl_fwd(d(pp), d(pr), B, G, 32, beta, out.t, klg.t, nseg)
    torch.cuda.synchronize()
    same_bits(dpp.value(), a1, "cat_kl_bwd dpp"); same_bits(dpr.value(), b1, "cat_kl_bwd dpr"); same_bits(out.value(), o1, "cat_kl_fwd out")


def test_cat_kl_and_plan_sampler_refuse_what_they_cannot_run(dev):
    from hulc2_amd import kernels as kn

    B, G = 4, 2
    z = torch.zeros(B, G * 16, device=dev)
    out, klg, dpp, dpr = out_flat(dev, 3), out_flat(dev, B * G), Guarded(dev, B, G * 32), Guarded(dev, B, G * 32)
    refused(lambda: kn.cat_kl_fwd(z, z, B, G, 16, 1.0, out.t, klg.t, 1), "hulc_cat_kl_fwd: class_size must be 32 (one 32-lane sub-wave per category)", out, klg)
    refused(lambda: kn.cat_kl_bwd(z, z, klg.t, B, G, 16, 1.0, 0.8, torch.ones(1, device=dev), dpp.t, dpr.t, 1), "hulc_cat_kl_bwd: class_size must be 32", dpp, dpr)
    z = torch.zeros(B, G * 32, device=dev)
    refused(lambda: kn.cat_kl_fwd(z, z, B, G, 32, 1.0, out.t, klg.t, 3), "hulc_cat_kl_fwd: the batch must split evenly into nseg segments", out, klg)
    refused(lambda: kn.cat_kl_bwd(z, z, klg.t, B, G, 32, 1.0, 0.8, torch.ones(3, device=dev), dpp.t, dpr.t, 3),
            "hulc_cat_kl_bwd: the batch must split evenly into nseg segments", dpp, dpr)
    idx = torch.zeros(B * G, dtype=torch.long, device=dev)
    refused(lambda: kn.plan_sample_fwd(z, idx, 0, B * G, 16, None, dpp.t), "hulc_plan_sample_fwd: class_size must be 32", dpp)
    refused(lambda: kn.plan_sample_bwd(z, z, B * G, 16, dpp.t), "hulc_plan_sample_bwd: class_size must be 32", dpp)


# ------------------------------------------------------------------------------------------------
# plan sampler
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NG", [1, 7, 8, 9, 2048])                  # 8 groups per workgroup: below, at and above one workgroup; the model's 64 x 32
def test_plan_sample_fwd_with_injected_indices(dev, NG):
    from hulc2_amd import kernels as kn

    g = _gen("plan", NG)
    idx = torch.randint(0, 32, (NG,), generator=g)
    idx[0], idx[-1] = 31, 0
    logits = torch.randn(NG, 32, generator=g).to(dev)
    plan, idx_out = Guarded(dev, NG, 32), out_flat(dev, NG, torch.int64)
    kn.plan_sample_fwd(logits, idx.to(dev), 0, NG, 32, idx_out.t, plan.t)
    torch.cuda.synchronize()
    plan.assert_guards("plan"); idx_out.assert_guards("idx_out")
    assert torch.equal(plan.value().cpu(), F.one_hot(idx, 32).float()), "one-hot rows, bit for bit"
    assert torch.equal(idx_out.value().cpu().reshape(-1), idx)


@pytest.mark.parametrize("NG,accumulate,spread", [(1, False, 1.0), (7, True, 1.0), (9, False, 30.0), (2048, True, 1.0), (2048, False, 30.0)])
def test_plan_sample_bwd(dev, NG, accumulate, spread):
    """straight-through estimator: dlogits = softmax Jacobian^T dplan = p * (dplan - <p, dplan>)"""
    from hulc2_amd import kernels as kn

    g = _gen("planb", NG, accumulate)
    logits, dplan, d0 = rnd(_randn(g, NG, 32) * spread, F32), rnd(_randn(g, NG, 32), F32), rnd(_randn(g, NG, 32), F32)
    dl = Guarded(dev, NG, 32, init=d0)

    def ref(dt):
        p = torch.softmax(logits.to(dt), -1)
        gd = dplan.to(dt)
        return p * (gd - (p * gd).sum(-1, keepdim=True)) + (d0.to(dt) if accumulate else 0)

    def run():
        dl.t.copy_(d0.float())
        kn.plan_sample_bwd(logits.float().to(dev), dplan.float().to(dev), NG, 32, dl.t, accumulate=accumulate)
        torch.cuda.synchronize()
        return dl.value()

    v1 = run()
    dl.assert_guards("dlogits")
    compare("plan_sample_bwd", "dlogits", v1, ref(torch.float64), ref(F32), MARGIN["LIBM"], grad=True)
    same_bits(run(), v1, "plan_sample_bwd")


# ------------------------------------------------------------------------------------------------
# contrastive loss
# ------------------------------------------------------------------------------------------------
LS_CLAMP = math.log(100.0)          # the reference clamps logit_scale at ln(100) (hulc2.py: logit_scale.data.clamp_(0, np.log(100)))

# M, row0, use pattern, logit_scale
CLIP = [
    (1, 0, "all", 0.5),             # one row: both cross-entropies are 0, every gradient 0
    (2, 0, "all", 0.5),             # (not at the clamp: with two aligned rows the off-diagonal probabilities are ~e^-50 there, and float64
                                    #  autograd's softmax - onehot, 1 - 2e-22 rounded to 1, is no reference for the gradients any more)
    (2, 1, "all", 0.5),             # row0 = M - 1: a single participating row
    (3, 1, "alt", LS_CLAMP),
    (64, 0, "alt", 0.5),            # every other row masked out
    (64, 32, "all", LS_CLAMP),      # the benchmark's call: the language rows are the second half of the stacked batch
    (64, 63, "one", 0.5),
    (127, 1, "all", LS_CLAMP),      # odd sizes: the M * M loops end inside a wave
    (127, 0, "one", LS_CLAMP),      # a single row taking part among 127
    (128, 0, "all", LS_CLAMP),      # the most rows the kernel takes (132 KB of LDS), sharpest logits
    (128, 127, "all", 0.5),
    (128, 1, "alt", 0.5),
    (64, 0, "none", 0.5),           # nobody takes part: loss 0, row count 1, every gradient 0
]


def _clip_ref(im, tx, use, ls, row0):
    """Hulc2.clip_auxiliary_loss on already-projected features: rows row0.. masked by `use`, both directions of the cross-entropy"""
    a, b = im[row0:][use], tx[row0:][use]
    a, b = a / a.norm(dim=-1, keepdim=True), b / b.norm(dim=-1, keepdim=True)
    logits = ls.exp() * a @ b.t()
    labels = torch.arange(logits.shape[0])
    return (F.cross_entropy(logits, labels) + F.cross_entropy(logits.t(), labels)) / 2


@pytest.mark.parametrize("M,row0,pattern,ls", CLIP)
def test_clip_loss(dev, M, row0, pattern, ls):
    from hulc2_amd import kernels as kn

    g = _gen("clip", M, row0, pattern)
    im, tx = rnd(_randn(g, M, 32) * 2.0, F32), rnd(_randn(g, M, 32) * 0.5, F32)
    tx = rnd(tx + 0.5 * im / 2.0, F32)                               # matching pairs correlate, as trained features do
    n = M - row0
    use = {"all": torch.ones(n, dtype=torch.bool), "none": torch.zeros(n, dtype=torch.bool), "alt": torch.arange(n) % 2 == 0,
           "one": torch.arange(n) == n // 2}[pattern]
    cnt = int(use.sum())
    lsd, gout = torch.tensor([ls], dtype=torch.float64), rnd(torch.tensor([1.7], dtype=torch.float64), F32)
    lsd = rnd(lsd, F32)
    d = lambda t: t.float().to(dev)
    used = use.to(torch.uint8).to(dev)
    out = out_flat(dev, 2)
    kn.clip_loss_fwd(d(im), d(tx), used, d(lsd), M, 32, out.t, row0)
    torch.cuda.synchronize()
    out.assert_guards("out")
    o1 = out.value().reshape(-1)
    assert float(o1[1]) == (cnt if cnt else 1), "the number of rows taking part (1 when there are none)"
    dim, dtx, dsc = Guarded(dev, M, 32), Guarded(dev, M, 32), out_flat(dev, 1)
    args = (d(im), d(tx), used, d(lsd), M, 32, d(gout), dim.t, dtx.t, dsc.t, row0)
    kn.clip_loss_bwd(*args)
    torch.cuda.synchronize()
    dim.assert_guards("dim"); dtx.assert_guards("dtx"); dsc.assert_guards("dscale")
    g1 = (dim.value(), dtx.value(), dsc.value())
    off = torch.ones(M, dtype=torch.bool)
    off[row0:] = ~use
    assert (g1[0].cpu()[off] == 0).all() and (g1[1].cpu()[off] == 0).all(), "rows below row0 and masked rows get exact zeros"
    if cnt == 0:
        assert float(o1[0]) == 0.0 and float(g1[2]) == 0.0
    else:
        def ref(dt):
            a, b, s = (t.detach().clone().to(dt).requires_grad_() for t in (im, tx, lsd))
            loss = _clip_ref(a, b, use, s, row0)
            (loss * gout.to(dt)).sum().backward()
            return loss.detach(), a.grad, b.grad, s.grad

        r, f = ref(torch.float64), ref(F32)
        if cnt == 1:
            assert float(r[0]) == 0.0
        m = MARGIN["CLIP_CLAMP" if ls == LS_CLAMP else "LIBM"]
        compare("clip_loss_fwd", "loss", o1[0], r[0], f[0], m)
        compare("clip_loss_bwd", "dim", g1[0], r[1], f[1], m, grad=True)
        compare("clip_loss_bwd", "dtx", g1[1], r[2], f[2], m, grad=True)
        compare("clip_loss_bwd", "dscale", g1[2], r[3], f[3], MARGIN["CLIP_CLAMP_DSCALE" if ls == LS_CLAMP else "LIBM"])
    out.t.fill_(float("nan")); dim.t.fill_(float("nan")); dtx.t.fill_(float("nan")); dsc.t.fill_(float("nan"))
    kn.clip_loss_fwd(d(im), d(tx), used, d(lsd), M, 32, out.t, row0)
    kn.clip_loss_bwd(*args)
    torch.cuda.synchronize()
    same_bits(out.value().reshape(-1), o1, "clip_loss_fwd")
    for a, b, nm in zip((dim.value(), dtx.value(), dsc.value()), g1, ("dim", "dtx", "dscale")):
        same_bits(a, b, "clip_loss_bwd " + nm)


def test_clip_loss_refuses_what_it_cannot_run(dev):
    from hulc2_amd import kernels as kn

    M = 129
    z, use, one = torch.ones(M, 32, device=dev), torch.ones(M, dtype=torch.uint8, device=dev), torch.ones(1, device=dev)
    out, dim, dtx, dsc = out_flat(dev, 2), Guarded(dev, M, 32), Guarded(dev, M, 32), out_flat(dev, 1)
    refused(lambda: kn.clip_loss_fwd(z, z, use, one, M, 32, out.t), "hulc_clip_loss_fwd: needs M <= 128, D == 32, 0 <= row0 < M", out)
    refused(lambda: kn.clip_loss_bwd(z, z, use, one, M, 32, one, dim.t, dtx.t, dsc.t), "hulc_clip_loss_bwd: needs M <= 128, D == 32, 0 <= row0 < M", dim, dtx, dsc)
    refused(lambda: kn.clip_loss_fwd(z, z, use, one, 64, 32, out.t, 64), "hulc_clip_loss_fwd: needs M <= 128, D == 32, 0 <= row0 < M", out)
    refused(lambda: kn.clip_loss_fwd(z, z, use, one, 64, 16, out.t), "hulc_clip_loss_fwd: needs M <= 128, D == 32, 0 <= row0 < M", out)


# ------------------------------------------------------------------------------------------------
# loss combiner, time-major actions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,with_clip", [(1, False), (2, True), (64, True), (64, False), (1, True)])
def test_loss_combine(dev, n, with_clip):
    """total = mean_m (act_m + kl_m) + beta * clip; out = {total, kl mean, action mean, beta * clip, per-modality act + kl ...}"""
    from hulc2_amd import kernels as kn

    g = _gen("combine", n, with_clip)
    beta = 3.0
    kls, acts, clip = rnd(_rand(g, n) * 0.1, F32), rnd(20.0 + _randn(g, n), F32), rnd(_rand(g, 1) * 4.0, F32)
    d = lambda t: t.float().to(dev)
    out = out_flat(dev, 4 + n)
    kn.loss_combine_fwd(d(kls), d(acts), d(clip) if with_clip else None, n, beta, out.t)
    torch.cuda.synchronize()
    out.assert_guards("out")

    def ref(dt):
        k, a, c = kls.to(dt), acts.to(dt), clip.to(dt)
        wc = beta * c if with_clip else torch.zeros(1, dtype=dt)
        return torch.cat([(a + k).sum(0, keepdim=True) / n + wc, k.sum(0, keepdim=True) / n, a.sum(0, keepdim=True) / n, wc, a + k])

    o1 = out.value()
    compare("loss_combine_fwd", "out", o1, ref(torch.float64), ref(F32), MARGIN["LIBM"])
    out.t.fill_(float("nan"))
    kn.loss_combine_fwd(d(kls), d(acts), d(clip) if with_clip else None, n, beta, out.t)
    torch.cuda.synchronize()
    same_bits(out.value(), o1, "loss_combine_fwd")
    gg = rnd(torch.tensor([1.3], dtype=torch.float64), F32)
    dk, da, dc = out_flat(dev, n), out_flat(dev, n), out_flat(dev, 1)
    kn.loss_combine_bwd(d(gg), n, beta, dk.t, da.t, dc.t if with_clip else None)
    torch.cuda.synchronize()
    dk.assert_guards("dkls"); da.assert_guards("dacts")
    want = (gg.float() / n).expand(n)
    assert torch.equal(dk.value().cpu().reshape(-1), want) and torch.equal(da.value().cpu().reshape(-1), want)
    if with_clip:
        dc.assert_guards("dclip")
        assert torch.equal(dc.value().cpu().reshape(-1), gg.float() * beta)
    else:
        dc.assert_untouched("dclip without a clip term")
    big = out_flat(dev, 4 + 65)
    refused(lambda: kn.loss_combine_fwd(torch.ones(65, device=dev), torch.ones(65, device=dev), None, 65, beta, big.t), "hulc_loss_combine_fwd: 1..64 modalities", big)
    refused(lambda: kn.loss_combine_bwd(d(gg), 65, beta, big.t, big.t, None), "hulc_loss_combine_bwd: 1..64 modalities", big)


def _euler_xyz(e):
    a, b, c = e.unbind(-1)
    ca, sa, cb, sb, cc, sc = a.cos(), a.sin(), b.cos(), b.sin(), c.cos(), c.sin()
    one, zero = torch.ones_like(a), torch.zeros_like(a)
    rx = torch.stack([one, zero, zero, zero, ca, -sa, zero, sa, ca], -1).reshape(*a.shape, 3, 3)
    ry = torch.stack([cb, zero, sb, zero, one, zero, -sb, zero, cb], -1).reshape(*a.shape, 3, 3)
    rz = torch.stack([cc, -sc, zero, sc, cc, zero, zero, zero, one], -1).reshape(*a.shape, 3, 3)
    return rx @ ry @ rz


def _world_to_tcp(act, obs):
    """gripper_control.py world_to_tcp_frame in the dtype of its arguments (rotation inverses as transposes)"""
    R = _euler_xyz(obs[..., 3:6])
    pos = (R.transpose(-1, -2) @ act[..., :3, None])[..., 0]
    Rn = _euler_xyz(obs[..., 3:6] + act[..., 3:6] * 0.01)
    m = Rn.transpose(-1, -2) @ R
    e = torch.stack([torch.atan2(-m[..., 1, 2], m[..., 2, 2]), torch.asin(m[..., 0, 2].clamp(-1, 1)), torch.atan2(-m[..., 0, 1], m[..., 0, 0])], -1)
    e = torch.where(e < -math.pi, e + 2 * math.pi, e)
    e = torch.where(e > math.pi, e - 2 * math.pi, e)
    return torch.cat([pos, e * 100.0, act[..., 6:7]], -1)


@pytest.mark.parametrize("nseg,B,S,obs_dim,to_tcp", [(1, 1, 1, 6, True), (2, 32, 32, 15, True), (3, 5, 7, 8, True), (4, 3, 33, 15, True),
                                                     (1, 64, 32, 15, False), (4, 5, 7, 15, False), (2, 1, 65, 6, False)])
def test_actions_time_major(dev, nseg, B, S, obs_dim, to_tcp):
    """out row (s * nseg * B + seg * B + b) = segment seg's action (b, s), moved to the tcp frame on the way or copied"""
    from hulc2_amd import functional as HF, kernels as kn

    g = _gen("atm", nseg, B, S, to_tcp)
    acts = [rnd(_rand(g, B, S, 7) * 2 - 1, F32) for _ in range(nseg)]
    obss = [rnd(_rand(g, B, S, obs_dim) * 2.4 - 1.2, F32) for _ in range(nseg)]
    out = Guarded(dev, S * nseg * B, 7)
    ad, od = [a.float().to(dev) for a in acts], [o.float().to(dev) for o in obss]
    kn.actions_time_major(ad, od, B, S, obs_dim, to_tcp, out.t)
    torch.cuda.synchronize()
    out.assert_guards("out")
    o1 = out.value()
    out.t.fill_(float("nan"))
    kn.actions_time_major(ad, od, B, S, obs_dim, to_tcp, out.t)
    torch.cuda.synchronize()
    same_bits(out.value(), o1, "actions_time_major")

    def ref(dt):
        rows = [(_world_to_tcp(a.to(dt), o.to(dt)) if to_tcp else a.to(dt)) for a, o in zip(acts, obss)]
        return torch.stack(rows, 0).permute(2, 0, 1, 3).reshape(S * nseg * B, 7)      # (seg, b, s) -> (s, seg, b)

    if to_tcp:
        compare("actions_time_major", "out", o1, ref(torch.float64), ref(F32), MARGIN["LIBM"])
        w = HF.world_to_tcp_frame(ad[0], od[0])                     # the batch-major kernel computes the same rows
        torch.cuda.synchronize()
        assert torch.equal(o1.view(S, nseg, B, 7)[:, 0].permute(1, 0, 2), w)
    else:
        assert torch.equal(o1.cpu(), ref(F32)), "a copy"
    big = Guarded(dev, 5, 7)
    refused(lambda: kn.actions_time_major([ad[0]] * 5, [od[0]] * 5, 1, 1, obs_dim, to_tcp, big.t),
            "hulc_actions_time_major: 1..4 segments, robot_obs with the euler angles in columns 3:6", big)
