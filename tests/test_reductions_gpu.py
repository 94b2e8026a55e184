"""Kernel-level tests of csrc/pointwise.hip (spatial softmax, the LayerNorm family, sequence means, the unfused attention, the small
pointwise kernels) and of the chunk / cast kernels of csrc/optim.hip, each against its closed form in float64 torch at the shapes, types and
edges where the launchers switch kernels or loop shapes.  The pattern of a case and the tolerance rule are in tests/kcheck.py."""
import math

import pytest
import torch

from tests import kcheck as K
from tests.kcheck import Guarded, compare, out_flat, refused, rnd, same_bits

pytestmark = pytest.mark.gpu

# Margins of margin * max(e_ref, 2^-23), e_ref = the float32 CPU evaluation of the same formula against float64 (tests/kcheck.py).
#   FAST 16: kernels built on __expf / rsqrtf (spatial softmax, LayerNorm, attention).  The intrinsic is good to 1-2 ulp and the kernel adds
#            in another tree than torch's float32 CPU code; both are legitimate, each worth a few float32 roundings, and nothing larger is.
#   SUM   4: plain float32 sums, products and copies (sequence means, column fan-in, chunk sums, partial reductions): only the summation
#            order differs from the CPU's.
# A case that cannot meet its margin is a finding: it gets its own row here with the measured float32-CPU and GPU errors and the cause.
MARGIN = {"FAST": 16.0, "SUM": 4.0}

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    K.report("tests/test_reductions_gpu.py")


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
# spatial softmax
# ------------------------------------------------------------------------------------------------
# which kernel a shape selects (hulc_spatial_softmax_fwd / _bwd): asserted through the shape only, the library has no probe
def _ssm_fwd_target(HW, C, aligned):
    if C == 64 and aligned:
        return "regs" if 32 <= HW <= 448 else "online"
    return "generic"


def _ssm_bwd_target(C, aligned):
    return "bwd64" if C == 64 and aligned else "generic"


# HW, C, N, storage, T, family, lead, dx type, relu_mask, expected (fwd, bwd) kernel
SSM = [
    (441, 64, 3, BF, 1.0, "relu", 0, BF, True, ("regs", "bwd64")),          # the static camera's 21 x 21 map, the model's own call
    (49, 64, 64, BF, 1.0, "relu", 0, BF, True, ("regs", "bwd64")),          # the gripper camera's 7 x 7 map, a full batch of frames
    (32, 64, 1, F32, 0.25, "peaked", 0, F32, False, ("regs", "bwd64")),     # lower edge of the register kernel: one position per lane
    (448, 64, 1, F32, 4.0, "lastpos", 0, F32, True, ("regs", "bwd64")),     # upper edge: all 14 register slots of every lane live
    (441, 64, 3, F32, 1.0, "zero", 0, BF, True, ("regs", "bwd64")),         # an all-zero channel: uniform softmax, coordinates = map means
    (449, 64, 3, F32, 1.0, "lastpos", 0, F32, True, ("online", "bwd64")),   # one position past the register kernel: online merge
    (900, 64, 1, BF, 0.25, "peaked", 0, BF, False, ("online", "bwd64")),    # a 30 x 30 map, x / T up to 320: needs the running maximum
    (31, 64, 3, F32, 1.0, "zero", 0, F32, True, ("online", "bwd64")),       # HW < 32: one lane of wave 3 holds an EMPTY partial (-inf max)
    (16, 64, 1, BF, 4.0, "relu", 0, F32, True, ("online", "bwd64")),        # waves 2 and 3 entirely empty
    (1, 64, 3, F32, 1.0, "relu", 0, F32, False, ("online", "bwd64")),       # a single position: softmax = 1, coordinates = the map value
    (441, 64, 3, F32, 1.0, "relu", 1, F32, True, ("generic", "generic")),   # the same map as a view one element in: not 32-byte aligned
    (49, 64, 3, BF, 4.0, "lastpos", 1, BF, True, ("generic", "generic")),   # bf16 view one element in (2-byte offset)
    (49, 63, 3, BF, 1.0, "relu", 0, BF, True, ("generic", "generic")),      # C = 63: lane 63 idle, odd row pitch
    (900, 32, 1, F32, 0.25, "peaked", 0, F32, False, ("generic", "generic")),   # half the lanes, HW a multiple of 4
    (449, 1, 3, F32, 1.0, "lastpos", 0, BF, True, ("generic", "generic")),  # one channel, HW = 4 * 112 + 1: the last wave's share is short
    (31, 32, 64, BF, 4.0, "zero", 0, F32, True, ("generic", "generic")),    # HW not a multiple of 4, many frames
    (16, 63, 1, F32, 0.25, "relu", 0, F32, True, ("generic", "generic")),
    (1, 1, 1, F32, 1.0, "relu", 0, F32, False, ("generic", "generic")),     # the smallest call: waves 1..3 have no position at all
    (32, 32, 3, BF, 1.0, "peaked", 0, BF, True, ("generic", "generic")),
    (448, 63, 1, BF, 0.25, "lastpos", 0, F32, False, ("generic", "generic")),
    (441, 64, 3, F16, 1.0, "relu", 0, BF, True, ("regs", "bwd64")),         # the fp16 twin of the static map (precision site "a3")
    (441, 64, 1, F16, 0.25, "f16max", 0, F32, True, ("regs", "bwd64")),     # 65504, the largest finite half, at T = 0.25
    (900, 64, 3, F16, 1.0, "f16max", 0, F32, False, ("online", "bwd64")),   # the same through the online kernel
    (16, 64, 3, F16, 4.0, "peaked", 0, BF, True, ("online", "bwd64")),
]


def _ssm_last_share(HW, target, c):
    """the last position of the last wave's share (where a dominant value sits in the `lastpos` family).  generic: waves own contiguous
    quarters, the last share ends at HW - 1.  64-channel kernels: wave w owns positions p with (p % 32) // 8 == w, so wave 3's last
    position is the largest p < HW with p % 32 >= 24.  Even channels take the first, odd channels the second form (both when they agree)."""
    p64 = max((p for p in range(HW) if p % 32 >= 24), default=HW - 1)
    return HW - 1 if (c % 2 == 0 or target == "generic") else p64


def _ssm_input(g, N, HW, C, dtype, T, family, target):
    x = torch.relu(_randn(g, N, HW, C)) * 2.0                        # post-ReLU: about half exact zeros
    if family == "zero":
        x[:, :, 0] = 0.0
        if C > 2:
            x[N - 1, :, C - 1] = 0.0
    elif family == "peaked":
        x = 80.0 * _rand(g, N, HW, C) ** 4                           # x / T up to 80 / T: exp overflows float32 without the max subtraction
        x[:, HW // 2, :] = 80.0
    elif family == "lastpos":
        for c in range(C):
            x[:, _ssm_last_share(HW, target, c), c] = 30.0 * T + 3.0   # e^-30 against every other position: it alone decides the result
    elif family == "f16max":
        x = torch.relu(_randn(g, N, HW, C)) * 100.0
        for c in range(C):
            x[:, (7 * c + 3) % HW, c] = 65504.0
        x[:, HW - 1, 0] = 65504.0                                    # two equal maxima in channel 0
    return rnd(x, dtype)


def _ssm_ref_fwd(x, xmap, ymap, T):
    """softmax over the HW positions of x / T, expectations of the two maps; stats = (max, sum of exp(x / T - max))"""
    z = x * (1.0 / T)
    m = z.max(dim=1, keepdim=True).values
    e = torch.exp(z - m)
    s = e.sum(dim=1)
    ex, ey = (e * xmap[None, :, None]).sum(1) / s, (e * ymap[None, :, None]).sum(1) / s
    return torch.stack([ex, ey], -1).reshape(x.shape[0], -1), torch.stack([m[:, 0], s], -1)


def _ssm_ref_bwd(x, xmap, ymap, T, out, stats, dout, relu_mask):
    """dz[n][p][c] = (x > 0) * (1/T) * softmax_p * (gx * (xmap_p - ex) + gy * (ymap_p - ey)) from the saved (max, sum) and expectations"""
    N, HW, C = x.shape
    o, g = out.reshape(N, C, 2), dout.reshape(N, C, 2)
    p = torch.exp(x * (1.0 / T) - stats[:, None, :, 0]) / stats[:, None, :, 1]
    d = (1.0 / T) * p * (g[:, None, :, 0] * (xmap[None, :, None] - o[:, None, :, 0]) + g[:, None, :, 1] * (ymap[None, :, None] - o[:, None, :, 1]))
    return torch.where(x > 0, d, torch.zeros_like(d)) if relu_mask else d


@pytest.mark.parametrize("HW,C,N,dtype,T,family,lead,dx_dtype,relu_mask,expect", SSM)
def test_spatial_softmax(dev, HW, C, N, dtype, T, family, lead, dx_dtype, relu_mask, expect):
    from hulc2_amd import kernels as kn

    g = _gen("ssm", HW, C, N, family, lead)
    aligned = lead == 0
    assert (_ssm_fwd_target(HW, C, aligned), _ssm_bwd_target(C, aligned)) == expect
    x64 = _ssm_input(g, N, HW, C, dtype, T, family, expect[0])
    xmap = rnd(torch.linspace(-1, 1, HW, dtype=torch.float64), F32)
    ymap = rnd(torch.linspace(-1, 1, HW, dtype=torch.float64)[torch.randperm(HW, generator=g)] * 0.5 + 0.25, F32)
    xg = Guarded(dev, 1, N * HW * C, dtype, init=x64, lead=lead)            # (an input: the guard only provides the shifted pointer)
    assert (xg.t.data_ptr() % (32 if dtype == F32 else 16) == 0) == aligned
    xm, ym, Td = xmap.float().to(dev), ymap.float().to(dev), torch.tensor([T], device=dev)
    out, stats = out_flat(dev, N * 2 * C), out_flat(dev, N * C * 2)
    kn.spatial_softmax_fwd(xg.t, N, HW, C, xm, ym, Td, out.t, stats.t)
    torch.cuda.synchronize()
    out.assert_guards("out"); stats.assert_guards("stats")
    o1, s1 = out.value(), stats.value()
    r_out, r_st = _ssm_ref_fwd(x64, xmap, ymap, T)
    f_out, f_st = _ssm_ref_fwd(x64.float(), xmap.float(), ymap.float(), T)
    kname = "spatial_softmax_fwd/" + expect[0]
    compare(kname, "out", o1, r_out, f_out, MARGIN["FAST"])
    st = s1.view(N, C, 2).double().cpu()
    assert torch.equal(st[..., 0], r_st[..., 0]), "stats: the maximum of x / T is exact in float32 (T is a power of two)"
    compare(kname, "stats.sum", st[..., 1], r_st[..., 1], f_st[..., 1], MARGIN["FAST"])
    o = o1.view(N, C, 2).double().cpu()
    assert (o[..., 0] >= xmap.min()).all() and (o[..., 0] <= xmap.max()).all(), "x coordinate outside [min(xmap), max(xmap)]"
    assert (o[..., 1] >= ymap.min()).all() and (o[..., 1] <= ymap.max()).all(), "y coordinate outside [min(ymap), max(ymap)]"
    if family == "zero":                  # uniform softmax: the coordinates are the map means
        zc = o[:, 0]
        assert (zc[:, 0] - xmap.mean()).abs().max() <= 16 * K.EPS32 and (zc[:, 1] - ymap.mean()).abs().max() <= 16 * K.EPS32
    out.t.fill_(float("nan")); stats.t.fill_(float("nan"))
    kn.spatial_softmax_fwd(xg.t, N, HW, C, xm, ym, Td, out.t, stats.t)
    torch.cuda.synchronize()
    same_bits(out.value(), o1, "spatial_softmax_fwd out"); same_bits(stats.value(), s1, "spatial_softmax_fwd stats")

    # backward from the float32-rounded reference (out, stats), so the forward's own error is not measured a second time
    out32, st32 = rnd(r_out, F32), rnd(r_st, F32)
    dout = rnd(_randn(g, N, 2 * C), F32)
    dx = Guarded(dev, 1, N * HW * C, dx_dtype, lead=lead)
    args = (xg.t, N, HW, C, xm, ym, Td, out32.float().to(dev), st32.float().to(dev), dout.float().to(dev), dx.t)
    kn.spatial_softmax_bwd(*args, relu_mask=relu_mask)
    torch.cuda.synchronize()
    dx.assert_guards("dx")
    d1 = dx.value()
    r_dx = _ssm_ref_bwd(x64, xmap, ymap, T, out32, st32, dout, relu_mask)
    f_dx = _ssm_ref_bwd(x64.float(), xmap.float(), ymap.float(), T, out32.float(), st32.float(), dout.float(), relu_mask)
    compare("spatial_softmax_bwd/" + expect[1], "dx", d1, r_dx, f_dx, MARGIN["FAST"], grad=True, out_dtype=dx_dtype)
    if relu_mask:
        assert (d1.view(N, HW, C).cpu()[x64 <= 0] == 0).all(), "the ReLU mask leaves exact zeros"
    dx.t.fill_(float("nan"))
    kn.spatial_softmax_bwd(*args, relu_mask=relu_mask)
    torch.cuda.synchronize()
    same_bits(dx.value(), d1, "spatial_softmax_bwd dx")


def test_spatial_softmax_refuses_what_it_cannot_run(dev):
    from hulc2_amd import kernels as kn

    N, HW = 2, 16
    xm, Td = torch.linspace(-1, 1, HW, device=dev), torch.ones(1, device=dev)
    for C, dtype, msg_f, msg_b in [(65, F32, "hulc_spatial_softmax_fwd: C must be in 1..64 (lane = channel)", "hulc_spatial_softmax_bwd: C must be in 1..64"),
                                   (32, F16, "hulc_spatial_softmax_fwd: an fp16 map has 64 channels, 16-byte aligned",
                                    "hulc_spatial_softmax_bwd: an fp16 map has 64 channels, 16-byte aligned")]:
        x = torch.ones(N, HW, C, device=dev, dtype=dtype)
        out, stats, dx = out_flat(dev, N * 2 * C), out_flat(dev, N * C * 2), out_flat(dev, N * HW * C)
        refused(lambda: kn.spatial_softmax_fwd(x, N, HW, C, xm, xm, Td, out.t, stats.t), msg_f, out, stats)
        o, s, d = torch.zeros(N, 2 * C, device=dev), torch.ones(N, C, 2, device=dev), torch.ones(N, 2 * C, device=dev)
        refused(lambda: kn.spatial_softmax_bwd(x, N, HW, C, xm, xm, Td, o, s, d, dx.t), msg_b, dx)
    # an fp16 map one element in (not 16-byte aligned): no kernel reads halves one by one
    xg = Guarded(dev, 1, N * HW * 64, F16, init=torch.ones(N * HW * 64), lead=1)
    out, stats = out_flat(dev, N * 128), out_flat(dev, N * 128)
    refused(lambda: kn.spatial_softmax_fwd(xg.t, N, HW, 64, xm, xm, Td, out.t, stats.t), "hulc_spatial_softmax_fwd: an fp16 map has 64 channels, 16-byte aligned",
            out, stats)


# ------------------------------------------------------------------------------------------------
# LayerNorm family
# ------------------------------------------------------------------------------------------------
EPS_LN = 1e-5


def _ln_rows(g, R, D, family):
    """normal: N(0, 1) * 1.5 + 0.3.  mean1e3: every row has mean 1e3 and unit spread (E[x^2] - mean^2 would lose every digit).  const: every
    third row is one constant with few mantissa bits (sums of it are exact in any order, so the variance is exactly 0 in float32 as in
    float64 and y = beta).  outlier: one row carries a single 1e4 among unit values."""
    x = _randn(g, R, D) * 1.5 + 0.3
    if family == "mean1e3":
        x = _randn(g, R, D) + 1e3
    elif family == "const":
        consts = torch.tensor([0.75, -3.0, 0.0, 1024.0, -0.046875], dtype=torch.float64)
        for r in range(0, R, 3):
            x[r] = consts[(r // 3) % 5]
    elif family == "outlier":
        x[R // 2, D // 2] = 1e4
    return rnd(x, F32)


def _ln_ref_fwd(x, o, gamma, beta):
    pre = x if o is None else x + o
    mean = pre.mean(-1, keepdim=True)
    var = ((pre - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS_LN)
    return pre, (pre - mean) * rstd * gamma + beta, mean[:, 0], rstd[:, 0]


def _ln_ref_bwd(dy, pre, mean, rstd, gamma):
    """dpre = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma; dgamma = sum_r dy * xhat, dbeta = sum_r dy"""
    xh = (pre - mean[:, None]) * rstd[:, None]
    gg = dy * gamma
    dpre = rstd[:, None] * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    return dpre, (dy * xh).sum(0), dy.sum(0)


def _f(t):
    return t.float()


# R, D, residual branch, family, accumulate_params
LN = [
    (1, 1, False, "normal", False),        # one element: mean = x, variance 0, y = beta
    (3, 7, True, "normal", True),          # fewer rows than waves, fewer columns than lanes
    (4, 32, False, "const", False),        # exactly one workgroup of rows; rows of variance exactly 0
    (5, 63, True, "normal", False),        # one row into the second workgroup; lane 63 idle
    (1023, 64, False, "mean1e3", True),    # last row block short by one (4 rows per block up to 1024 rows)
    (1024, 65, True, "normal", False),     # the last size with 4 rows per block; one column in the second register
    (1025, 128, False, "outlier", True),   # first size with 5 rows per block: wave 0 takes two rows, the others one
    (2112, 192, True, "normal", False),    # 33 x 64 rows (a time-major batch), 9 rows per block, three registers per lane
    (4099, 255, False, "normal", True),    # 17 rows per block, last block of 2 rows; one column short of the widest row
    (4, 256, True, "mean1e3", False),      # the widest row the kernel takes
    (1024, 128, True, "const", True),      # the transformer's width at a row-block edge
    (5, 64, False, "outlier", False),
    (3, 255, True, "normal", False),
    (1025, 7, False, "normal", False),
]


@pytest.mark.parametrize("R,D,residual,family,accumulate", LN)
def test_layernorm_fwd_bwd(dev, R, D, residual, family, accumulate):
    from hulc2_amd import kernels as kn

    g = _gen("ln", R, D, family, residual)
    x = _ln_rows(g, R, D, family)
    o = rnd(_randn(g, R, D) * 0.5, F32) if residual else None
    if family == "const" and residual:
        o[::3] = 0.25                                               # keep those rows constant after the residual add
    gamma, beta = rnd(1.0 + 0.3 * _randn(g, D), F32), rnd(0.2 * _randn(g, D), F32)
    d = lambda t: None if t is None else t.float().to(dev)
    pre, y, mean, rstd = Guarded(dev, R, D), Guarded(dev, R, D), out_flat(dev, R), out_flat(dev, R)
    want_pre = residual or R % 2 == 1                                # pre_out is optional without a residual branch: both forms
    args = (d(x), d(o), 0.0, 0, d(gamma), d(beta), EPS_LN, R, D, pre.t if want_pre else None, y.t, mean.t, rstd.t)
    kn.layernorm_fwd(*args)
    torch.cuda.synchronize()
    for gd, nm in ((pre, "pre_out"), (y, "y"), (mean, "mean"), (rstd, "rstd")):
        gd.assert_guards(nm)
    if not want_pre:
        pre.assert_untouched("pre_out not asked for")
    r = _ln_ref_fwd(x, o, gamma, beta)
    f = _ln_ref_fwd(_f(x), None if o is None else _f(o), _f(gamma), _f(beta))
    got = (pre.value(), y.value(), mean.value(), rstd.value())
    for i, nm in enumerate(("pre_out", "y", "mean", "rstd")):
        if nm == "pre_out" and not want_pre:
            continue
        compare("layernorm_fwd", nm, got[i], r[i], f[i], MARGIN["FAST"])
    if family == "const":
        yy = got[1].double().cpu()
        assert torch.equal(yy[::3], beta.expand(R, D)[::3]), "a constant row has variance exactly 0: y = beta"
    y.t.fill_(float("nan")); mean.t.fill_(float("nan")); rstd.t.fill_(float("nan"))
    kn.layernorm_fwd(*args)
    torch.cuda.synchronize()
    same_bits(y.value(), got[1], "layernorm_fwd y"); same_bits(mean.value(), got[2], "mean"); same_bits(rstd.value(), got[3], "rstd")

    # backward from the float32-rounded reference statistics
    pre32, mean32, rstd32 = rnd(r[0], F32), rnd(r[2], F32), rnd(r[3], F32)
    dy = rnd(_randn(g, R, D), F32)
    dg0, db0 = rnd(_randn(g, D) * 3.0, F32), rnd(_randn(g, D) * 3.0, F32)          # non-zero starting values of the accumulated form
    dpre, do_out = Guarded(dev, R, D), Guarded(dev, R, D)
    dgamma, dbeta = out_flat(dev, D, init=dg0), out_flat(dev, D, init=db0)

    def run():
        dgamma.t.copy_(dg0.float().reshape(1, D)); dbeta.t.copy_(db0.float().reshape(1, D))
        kn.layernorm_bwd(d(dy), d(pre32), d(mean32), d(rstd32), d(gamma), R, D, dpre.t, do_out.t if residual else None, 0.0, 0, dgamma.t, dbeta.t,
                         accumulate_params=accumulate)
        torch.cuda.synchronize()
        return dpre.value(), do_out.value(), dgamma.value(), dbeta.value()

    b1 = run()
    for gd, nm in ((dpre, "dpre"), (do_out, "do_out"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        gd.assert_guards(nm)
    if not residual:
        do_out.assert_untouched("do_out not asked for")
    rb = _ln_ref_bwd(dy, pre32, mean32, rstd32, gamma)
    fb = _ln_ref_bwd(_f(dy), _f(pre32), _f(mean32), _f(rstd32), _f(gamma))
    acc = lambda t, t0, dt: t + (t0.to(dt) if accumulate else 0)
    compare("layernorm_bwd", "dpre", b1[0], rb[0], fb[0], MARGIN["FAST"], grad=True)
    if residual:
        assert torch.equal(b1[1], b1[0]), "without dropout the branch gradient is dpre itself"
    compare("layernorm_bwd", "dgamma", b1[2], acc(rb[1], dg0, torch.float64), acc(fb[1], dg0, F32), MARGIN["FAST"], grad=True)
    compare("layernorm_bwd", "dbeta", b1[3], acc(rb[2], db0, torch.float64), acc(fb[2], db0, F32), MARGIN["FAST"], grad=True)
    b2 = run()
    for a, b, nm in zip(b1, b2, ("dpre", "do_out", "dgamma", "dbeta")):
        if nm != "do_out" or residual:
            same_bits(b, a, "layernorm_bwd " + nm)


# R, D, n_o, extra o_stride
SLAB = [
    (5, 63, 1, 1),          # a single slab: the loop body never runs
    (4, 128, 2, 7),         # tail only
    (1025, 64, 4, 64),      # tail of three (the unrolled trip needs slabs 1..4)
    (3, 256, 5, 1),         # exactly one unrolled trip, no tail
    (7, 192, 8, 5),         # one trip + tail of three
    (2112, 128, 16, 128),   # the fused feed-forward's 16 slices at the transformer's width: three trips + tail of three
    (1, 1, 16, 3),
]


@pytest.mark.parametrize("R,D,n_o,extra", SLAB)
def test_layernorm_slab_fwd(dev, R, D, n_o, extra):
    from hulc2_amd import kernels as kn

    g = _gen("slab", R, D, n_o)
    x = rnd(_randn(g, R, D), F32)
    stride = R * D + extra                                           # o_stride > R * D: the gap holds NaN, a read of it poisons the row
    slabs = torch.full((n_o, stride), float("nan"), dtype=torch.float64)
    slabs[:, :R * D] = rnd(_randn(g, n_o, R * D) * (1.0 + torch.arange(n_o, dtype=torch.float64)[:, None]), F32)
    gamma, beta = rnd(1.0 + 0.3 * _randn(g, D), F32), rnd(0.2 * _randn(g, D), F32)
    d = lambda t: t.float().to(dev)
    pre, y, mean, rstd = Guarded(dev, R, D), Guarded(dev, R, D), out_flat(dev, R), out_flat(dev, R)
    args = (d(x), d(slabs), n_o, stride, 0.0, 0, d(gamma), d(beta), EPS_LN, R, D, pre.t, y.t, mean.t, rstd.t)
    kn.layernorm_slab_fwd(*args)
    torch.cuda.synchronize()
    for gd, nm in ((pre, "pre_out"), (y, "y"), (mean, "mean"), (rstd, "rstd")):
        gd.assert_guards(nm)

    def ref(dt):
        o = slabs[0, :R * D].to(dt)
        for s in range(1, n_o):                                      # the kernel's order: slab by slab
            o = o + slabs[s, :R * D].to(dt)
        return _ln_ref_fwd(x.to(dt), o.view(R, D), gamma.to(dt), beta.to(dt))

    r, f = ref(torch.float64), ref(F32)
    got = (pre.value(), y.value(), mean.value(), rstd.value())
    for i, nm in enumerate(("pre_out", "y", "mean", "rstd")):
        compare("layernorm_slab_fwd", nm, got[i], r[i], f[i], MARGIN["FAST"])
    y.t.fill_(float("nan")); pre.t.fill_(float("nan"))
    kn.layernorm_slab_fwd(*args)
    torch.cuda.synchronize()
    same_bits(y.value(), got[1], "layernorm_slab_fwd y"); same_bits(pre.value(), got[0], "layernorm_slab_fwd pre_out")


# R, D, ld_y, ld_dy, accumulate
LN_LD = [
    (5, 64, 64, 64, False),        # pitch = width: the plain layout through the strided entry points
    (3, 64, 65, 128, True),        # one padding column (odd pitch) out, the camera encoders' 64 + 64 halves in
    (1025, 32, 64, 33, False),     # the gripper encoder's half-width block; 5 rows per block in the backward
    (4, 255, 510, 256, True),
    (1, 1, 2, 2, False),
    (1024, 128, 129, 256, True),
]


@pytest.mark.parametrize("R,D,ld_y,ld_dy,accumulate", LN_LD)
def test_layernorm_ld_forms(dev, R, D, ld_y, ld_dy, accumulate):
    from hulc2_amd import kernels as kn

    g = _gen("lnld", R, D, ld_y, ld_dy)
    x = _ln_rows(g, R, D, "normal")
    gamma, beta = rnd(1.0 + 0.3 * _randn(g, D), F32), rnd(0.2 * _randn(g, D), F32)
    d = lambda t: t.float().to(dev)
    y, mean, rstd = Guarded(dev, R, D, ld=ld_y), out_flat(dev, R), out_flat(dev, R)
    kn.layernorm_fwd_ld(d(x), d(gamma), d(beta), EPS_LN, R, D, y.t, ld_y, mean.t, rstd.t)
    torch.cuda.synchronize()
    y.assert_guards("y (padding columns and guard bands)"); mean.assert_guards("mean"); rstd.assert_guards("rstd")
    r, f = _ln_ref_fwd(x, None, gamma, beta), _ln_ref_fwd(_f(x), None, _f(gamma), _f(beta))
    got = (None, y.value(), mean.value(), rstd.value())
    for i, nm in ((1, "y"), (2, "mean"), (3, "rstd")):
        compare("layernorm_fwd_ld", nm, got[i], r[i], f[i], MARGIN["FAST"])
    y.t.fill_(float("nan"))
    kn.layernorm_fwd_ld(d(x), d(gamma), d(beta), EPS_LN, R, D, y.t, ld_y, mean.t, rstd.t)
    torch.cuda.synchronize()
    same_bits(y.value(), got[1], "layernorm_fwd_ld y")

    mean32, rstd32 = rnd(r[2], F32), rnd(r[3], F32)
    dy = rnd(_randn(g, R, D), F32)
    dyg = Guarded(dev, R, D, ld=ld_dy, init=dy)                      # the incoming gradient is a block of a wider tensor; its padding is NaN
    dg0, db0 = rnd(_randn(g, D), F32), rnd(_randn(g, D), F32)
    dpre, dgamma, dbeta = Guarded(dev, R, D), out_flat(dev, D), out_flat(dev, D)

    def run():
        dgamma.t.copy_(dg0.float().reshape(1, D)); dbeta.t.copy_(db0.float().reshape(1, D))
        kn.layernorm_bwd_ld(dyg.t, ld_dy, d(x), d(mean32), d(rstd32), d(gamma), R, D, dpre.t, dgamma.t, dbeta.t, accumulate_params=accumulate)
        torch.cuda.synchronize()
        return dpre.value(), dgamma.value(), dbeta.value()

    b1 = run()
    dpre.assert_guards("dpre"); dgamma.assert_guards("dgamma"); dbeta.assert_guards("dbeta"); dyg.assert_guards("dy is an input")
    rb, fb = _ln_ref_bwd(dy, x, mean32, rstd32, gamma), _ln_ref_bwd(_f(dy), _f(x), _f(mean32), _f(rstd32), _f(gamma))
    acc = lambda t, t0, dt: t + (t0.to(dt) if accumulate else 0)
    compare("layernorm_bwd_ld", "dpre", b1[0], rb[0], fb[0], MARGIN["FAST"], grad=True)
    compare("layernorm_bwd_ld", "dgamma", b1[1], acc(rb[1], dg0, torch.float64), acc(fb[1], dg0, F32), MARGIN["FAST"], grad=True)
    compare("layernorm_bwd_ld", "dbeta", b1[2], acc(rb[2], db0, torch.float64), acc(fb[2], db0, F32), MARGIN["FAST"], grad=True)
    b2 = run()
    for a, b, nm in zip(b1, b2, ("dpre", "dgamma", "dbeta")):
        same_bits(b, a, "layernorm_bwd_ld " + nm)


def test_layernorm_refuses_what_it_cannot_run(dev):
    from hulc2_amd import kernels as kn

    R, D = 4, 257
    z = lambda *s: torch.ones(*s, device=dev)
    pre, y, mean, rstd, dpre = Guarded(dev, R, D), Guarded(dev, R, D), out_flat(dev, R), out_flat(dev, R), Guarded(dev, R, D)
    dg, db = out_flat(dev, D), out_flat(dev, D)
    refused(lambda: kn.layernorm_fwd(z(R, D), None, 0.0, 0, z(D), z(D), EPS_LN, R, D, pre.t, y.t, mean.t, rstd.t),
            "hulc_layernorm_fwd: D must be in 1..256", pre, y, mean, rstd)
    refused(lambda: kn.layernorm_slab_fwd(z(R, D), z(2, R * D), 2, R * D, 0.0, 0, z(D), z(D), EPS_LN, R, D, pre.t, y.t, mean.t, rstd.t),
            "hulc_layernorm_slab_fwd: D must be in 1..256, n_o >= 1", pre, y, mean, rstd)
    refused(lambda: kn.layernorm_bwd(z(R, D), z(R, D), z(R), z(R), z(D), R, D, dpre.t, None, 0.0, 0, dg.t, db.t),
            "hulc_layernorm_bwd: D must be in 1..256", dpre, dg, db)
    refused(lambda: kn.layernorm_fwd_ld(z(R, D), z(D), z(D), EPS_LN, R, D, y.t, D, mean.t, rstd.t),
            "hulc_layernorm_fwd_ld: D must be in 1..256, ld_y >= D", y, mean, rstd)
    refused(lambda: kn.layernorm_bwd_ld(z(R, D), D, z(R, D), z(R), z(R), z(D), R, D, dpre.t, dg.t, db.t),
            "hulc_layernorm_bwd_ld: D must be in 1..256, ld_dy >= D", dpre, dg, db)
    D = 64                                                           # a pitch narrower than the row
    y = Guarded(dev, R, D)
    refused(lambda: kn.layernorm_fwd_ld(z(R, D), z(D), z(D), EPS_LN, R, D, y.t, D - 1, mean.t, rstd.t),
            "hulc_layernorm_fwd_ld: D must be in 1..256, ld_y >= D", y, mean, rstd)
    dpre, dg, db = Guarded(dev, R, D), out_flat(dev, D), out_flat(dev, D)
    refused(lambda: kn.layernorm_bwd_ld(z(R, D), D - 1, z(R, D), z(R), z(R), z(D), R, D, dpre.t, dg.t, db.t),
            "hulc_layernorm_bwd_ld: D must be in 1..256, ld_dy >= D", dpre, dg, db)
    yw = Guarded(dev, 2, 1025)
    refused(lambda: kn.ln_wide_fwd(z(2, 1025), None, z(1025), z(1025), EPS_LN, 2, 1025, yw.t), "hulc_ln_wide_fwd: needs R > 0 and 0 < D <= 1024", yw)
    refused(lambda: kn.ln_partial_reduce_multi(z(9, 2, 2, 8), 2, 8, [dg.t] * 9, [db.t] * 9, [False] * 9), "hulc_ln_partial_reduce_multi: 1..8 LayerNorms", dg, db)


# P, D, accumulate
PARTIAL = [
    (1, 1, False),          # one partial row: 15 of the 16 row slices are empty
    (15, 65, True),         # fewer partial rows than slices; a second column block of one column
    (16, 128, False),       # one row per slice
    (17, 128, True),        # two rows per slice: the last slices are empty (per = 2, 9 slices used)
    (100, 7, False),
    (257, 256, True),       # the transformer block's largest partial count (4099 rows at 16 per block), widest row
]


@pytest.mark.parametrize("P,D,accumulate", PARTIAL)
def test_ln_partial_reduce(dev, P, D, accumulate):
    from hulc2_amd import kernels as kn

    g = _gen("lnp", P, D)
    part = rnd(_randn(g, P, 2, D), F32)
    dg0, db0 = rnd(_randn(g, D), F32), rnd(_randn(g, D), F32)
    dg, db = out_flat(dev, D, init=dg0), out_flat(dev, D, init=db0)
    kn.ln_partial_reduce(part.float().to(dev), P, D, dg.t, db.t, accumulate=accumulate)
    torch.cuda.synchronize()
    dg.assert_guards("dgamma"); db.assert_guards("dbeta")
    for gd, col, t0, nm in ((dg, 0, dg0, "dgamma"), (db, 1, db0, "dbeta")):
        r = part[:, col].sum(0) + (t0 if accumulate else 0)
        f = part[:, col].float().sum(0) + (t0.float() if accumulate else 0)
        compare("ln_partial_reduce", nm, gd.value(), r, f, MARGIN["SUM"], grad=True)
    a1, b1 = dg.value(), db.value()
    dg.t.copy_(dg0.float().reshape(1, D)); db.t.copy_(db0.float().reshape(1, D))
    kn.ln_partial_reduce(part.float().to(dev), P, D, dg.t, db.t, accumulate=accumulate)
    torch.cuda.synchronize()
    same_bits(dg.value(), a1, "ln_partial_reduce dgamma"); same_bits(db.value(), b1, "ln_partial_reduce dbeta")


@pytest.mark.parametrize("n,P,D", [(1, 17, 65), (3, 33, 128), (8, 5, 7)])      # one, a transformer layer's count, the most the launcher takes
def test_ln_partial_reduce_multi(dev, n, P, D):
    from hulc2_amd import kernels as kn

    g = _gen("lnpm", n, P, D)
    part = rnd(_randn(g, n, P, 2, D), F32)
    accs = [i % 2 == 1 for i in range(n)]
    g0 = [rnd(_randn(g, 2, D), F32) for _ in range(n)]
    dgs = [out_flat(dev, D, init=g0[i][0]) for i in range(n)]
    dbs = [out_flat(dev, D, init=g0[i][1]) for i in range(n)]
    kn.ln_partial_reduce_multi(part.float().to(dev), P, D, [t.t for t in dgs], [t.t for t in dbs], accs)
    torch.cuda.synchronize()
    single = out_flat(dev, D), out_flat(dev, D)
    for i in range(n):
        for gd, col, nm in ((dgs[i], 0, "dgamma"), (dbs[i], 1, "dbeta")):
            gd.assert_guards(f"{nm}[{i}]")
            r = part[i, :, col].sum(0) + (g0[i][col] if accs[i] else 0)
            f = part[i, :, col].float().sum(0) + (g0[i][col].float() if accs[i] else 0)
            compare("ln_partial_reduce_multi", f"{nm}[{i}]", gd.value(), r, f, MARGIN["SUM"], grad=True)
        # the same summation order as the single form
        single[0].t.copy_(g0[i][0].float().reshape(1, D)); single[1].t.copy_(g0[i][1].float().reshape(1, D))
        kn.ln_partial_reduce(part[i].float().to(dev), P, D, single[0].t, single[1].t, accumulate=accs[i])
        torch.cuda.synchronize()
        same_bits(dgs[i].value(), single[0].value(), "multi against single dgamma"); same_bits(dbs[i].value(), single[1].value(), "multi against single dbeta")


@pytest.mark.parametrize("R,add", [(1, False), (5, True), (64, True), (3, False)])      # the sentence encoder's width, ragged row counts
def test_ln_wide_fwd(dev, R, add):
    from hulc2_amd import kernels as kn

    D = 384
    g = _gen("lnw", R, add)
    x = rnd(_randn(g, R, D), F32)
    a = rnd(_randn(g, R, D) * 0.5, F32) if add else None
    gamma, beta = rnd(1.0 + 0.3 * _randn(g, D), F32), rnd(0.2 * _randn(g, D), F32)
    d = lambda t: None if t is None else t.float().to(dev)
    y = Guarded(dev, R, D)
    kn.ln_wide_fwd(d(x), d(a), d(gamma), d(beta), 1e-12, R, D, y.t)
    torch.cuda.synchronize()
    y.assert_guards("y")

    def ref(dt):
        pre = x.to(dt) + (a.to(dt) if add else 0)
        mean = pre.mean(-1, keepdim=True)
        var = ((pre - mean) ** 2).mean(-1, keepdim=True)
        return (pre - mean) / torch.sqrt(var + 1e-12) * gamma.to(dt) + beta.to(dt)

    y1 = y.value()
    compare("ln_wide_fwd", "y", y1, ref(torch.float64), ref(F32), MARGIN["FAST"])
    y.t.fill_(float("nan"))
    kn.ln_wide_fwd(d(x), d(a), d(gamma), d(beta), 1e-12, R, D, y.t)
    torch.cuda.synchronize()
    same_bits(y.value(), y1, "ln_wide_fwd y")


# ------------------------------------------------------------------------------------------------
# the small ones
# ------------------------------------------------------------------------------------------------
# B, S, D, scale
SEQ = [
    (1, 1, 1, 1.0),         # single everything
    (3, 7, 65, 0.5),        # ragged: tail of three after one unrolled trip
    (5, 32, 128, 1.0),      # the posterior's sequence mean
    (2, 33, 300, 2.0),      # B * D past one workgroup, S = 4 * 8 + 1
    (64, 4, 1, 1.0),        # single column; exactly one unrolled trip
    (1, 3, 257, 1.0),       # single row; tail only
]


@pytest.mark.parametrize("B,S,D,scale", SEQ)
def test_seq_mean_fwd_bwd(dev, B, S, D, scale):
    from hulc2_amd import kernels as kn

    g = _gen("seq", B, S, D)
    x = rnd(_randn(g, B, S, D), F32)
    y = Guarded(dev, B, D)
    kn.seq_mean_fwd(x.float().to(dev), y.t, B, S, D, scale)
    torch.cuda.synchronize()
    y.assert_guards("y")
    y1 = y.value()
    compare("seq_mean_fwd", "y", y1, scale * x.mean(1), scale * x.float().mean(1), MARGIN["SUM"])
    y.t.fill_(float("nan"))
    kn.seq_mean_fwd(x.float().to(dev), y.t, B, S, D, scale)
    torch.cuda.synchronize()
    same_bits(y.value(), y1, "seq_mean_fwd")
    dy = rnd(_randn(g, B, D), F32)
    dx = Guarded(dev, B * S, D)
    kn.seq_mean_bwd(dy.float().to(dev), dx.t, B, S, D)
    torch.cuda.synchronize()
    dx.assert_guards("dx")
    r = (dy / S)[:, None, :].expand(B, S, D)
    f = (dy.float() / S)[:, None, :].expand(B, S, D)
    d1 = dx.value()
    compare("seq_mean_bwd", "dx", d1, r, f, MARGIN["SUM"], grad=True)
    dx.t.fill_(float("nan"))
    kn.seq_mean_bwd(dy.float().to(dev), dx.t, B, S, D)
    torch.cuda.synchronize()
    same_bits(dx.value(), d1, "seq_mean_bwd")


# B, S, D, stride_b, stride_s, ldy, scale, storage
STRIDED = [
    (3, 7, 65, 7 * 70, 70, 65, 1.0, F32),           # batch-major rows with 5 padding columns
    (5, 33, 128, 256, 5 * 256, 130, 1.0 / 33, BF),  # time-major bf16 buffer, half of its 256 columns, padded destination
    (1, 1, 1, 1, 1, 1, 2.0, F32),
    (64, 4, 3, 3, 64 * 3, 4, 0.25, BF),             # time-major, exactly one unrolled trip
    (2, 3, 300, 1000, 300, 300, 1.0, F32),          # gap between batches, tail only
]


@pytest.mark.parametrize("B,S,D,stride_b,stride_s,ldy,scale,dtype", STRIDED)
def test_strided_seq_sum(dev, B, S, D, stride_b, stride_s, ldy, scale, dtype):
    from hulc2_amd import kernels as kn

    g = _gen("sss", B, S, D, stride_b)
    n = (B - 1) * stride_b + (S - 1) * stride_s + D
    buf = torch.full((n,), float("nan"), dtype=torch.float64)          # everything the sum must not touch is NaN
    x = rnd(_randn(g, B, S, D), dtype)
    idx = (torch.arange(B)[:, None, None] * stride_b + torch.arange(S)[None, :, None] * stride_s + torch.arange(D)[None, None, :]).reshape(-1)
    assert idx.unique().numel() == idx.numel(), "the test's own layout overlaps"
    buf[idx] = x.reshape(-1)
    y = Guarded(dev, B, D, ld=ldy)
    kn.strided_seq_sum(buf.to(dtype).to(dev), y.t, B, S, D, stride_b, stride_s, ldy, scale)
    torch.cuda.synchronize()
    y.assert_guards("y (padding columns and guard bands)")
    y1 = y.value()
    compare("strided_seq_sum", "y", y1, scale * x.sum(1), scale * x.float().sum(1), MARGIN["SUM"])
    y.t.fill_(float("nan"))
    kn.strided_seq_sum(buf.to(dtype).to(dev), y.t, B, S, D, stride_b, stride_s, ldy, scale)
    torch.cuda.synchronize()
    same_bits(y.value(), y1, "strided_seq_sum")


@pytest.mark.parametrize("B,S,D", [(1, 1, 1), (3, 7, 65), (5, 32, 128), (2, 33, 37)])       # ragged sizes; the transformer's own
def test_add_pos_fwd(dev, B, S, D):
    from hulc2_amd import kernels as kn

    g = _gen("pos", B, S, D)
    x, pos = rnd(_randn(g, B, S, D), F32), rnd(_randn(g, S + 3, D), F32)
    ids = torch.randperm(S + 3, generator=g)[:S]                     # permuted positions out of a longer table
    y = Guarded(dev, B * S, D)
    kn.add_pos_fwd(x.float().to(dev), pos.float().to(dev), ids.to(dev), y.t, B, S, D, 0.0, 0)
    torch.cuda.synchronize()
    y.assert_guards("y")
    ref = (x.float() + pos.float()[ids][None]).reshape(B * S, D)     # one float32 add per element: exact agreement
    assert torch.equal(y.value().cpu(), ref)


@pytest.mark.parametrize("n,dtype,scale", [(1, F32, 1.0), (255, BF, 1.25), (257, F32, 0.5), (4099, BF, 1.0 / 0.9), (65536 + 3, F32, 2.0)])
def test_relu_bwd(dev, n, dtype, scale):
    """dx = dy * (y > 0) * scale: exact zeros and negative zeros in y give exactly 0, every other element is one float32 product"""
    from hulc2_amd import kernels as kn

    g = _gen("relu", n)
    y = torch.relu(_randn(g, n))
    y[::5] = -0.0
    y[1::7] = -_rand(g, y[1::7].numel())                             # negative values: a saved pre-activation would have them
    y = y.to(dtype)
    dy = _randn(g, n).float()
    dx = out_flat(dev, n)
    kn.relu_bwd(dy.to(dev), y.to(dev), dx.t, n, scale)
    torch.cuda.synchronize()
    dx.assert_guards("dx")
    ref = torch.where(y.float() > 0, dy * torch.tensor(scale, dtype=F32), torch.zeros(n))
    assert torch.equal(dx.value().cpu().reshape(-1), ref)
    assert (dx.value().cpu().reshape(-1)[::5] == 0).all()


# N, S, D, n_last, lo, hi
FAN = [
    (1, 1, 1, 0, 0, 1),         # the smallest geometry, no last-frame rows
    (3, 7, 65, 1, 5, 60),       # a column slice starting inside the row
    (5, 32, 128, 5, 64, 128),   # the model's fan-out: the decoder sees the right half, every row feeds the goal encoder
    (4, 3, 37, 0, 36, 37),      # one-column slice at the end
    (2, 33, 70, 2, 0, 70),      # the whole row
]


@pytest.mark.parametrize("N,S,D,n_last,lo,hi", FAN)
def test_emb_fanout_fanin(dev, N, S, D, n_last, lo, hi):
    from hulc2_amd import kernels as kn

    g = _gen("fan", N, S, D, n_last, lo)
    E = hi - lo
    emb = rnd(_randn(g, N, S, D), F32)
    e0, el, ed = Guarded(dev, N, D), Guarded(dev, max(n_last, 1), D), Guarded(dev, S * N, E)
    kn.emb_fanout_fwd(emb.float().to(dev), N, S, D, n_last, lo, hi, e0.t, el.t if n_last else None, ed.t)
    torch.cuda.synchronize()
    e0.assert_guards("e0"); ed.assert_guards("edec_t")
    if n_last:
        el.assert_guards("elast")
        assert torch.equal(el.value().cpu()[:n_last], emb[:n_last, -1].float())
    else:
        el.assert_untouched("elast with n_last = 0")
    assert torch.equal(e0.value().cpu(), emb[:, 0].float())
    assert torch.equal(ed.value().cpu().view(S, N, E), emb[:, :, lo:hi].permute(1, 0, 2).float())
    g_rec, g0, gl, gd = (rnd(_randn(g, N, S, D), F32), rnd(_randn(g, N, D), F32), rnd(_randn(g, max(n_last, 1), D), F32), rnd(_randn(g, S, N, E), F32))
    d = lambda t: t.float().to(dev)
    for with_rec in (True, False):
        demb = Guarded(dev, N * S, D)
        kn.emb_fanin_bwd(d(g_rec) if with_rec else None, d(g0), d(gl) if n_last else None, d(gd), N, S, D, n_last, lo, hi, demb.t)
        torch.cuda.synchronize()
        demb.assert_guards("demb")

        def ref(dt):
            r = g_rec.to(dt).clone() if with_rec else torch.zeros(N, S, D, dtype=dt)
            r[:, 0] += g0.to(dt)
            if n_last:
                r[:n_last, -1] += gl.to(dt)[:n_last]
            r[:, :, lo:hi] += gd.to(dt).permute(1, 0, 2)
            return r

        d1 = demb.value()
        compare("emb_fanin_bwd", "demb", d1, ref(torch.float64), ref(F32), MARGIN["SUM"], grad=True)
        demb.t.fill_(float("nan"))
        kn.emb_fanin_bwd(d(g_rec) if with_rec else None, d(g0), d(gl) if n_last else None, d(gd), N, S, D, n_last, lo, hi, demb.t)
        torch.cuda.synchronize()
        same_bits(demb.value(), d1, "emb_fanin_bwd")
    z = Guarded(dev, N, D)
    refused(lambda: kn.emb_fanout_fwd(d(emb), N, S, D, N + 1, lo, hi, z.t, z.t, z.t), "hulc_emb_fanout_fwd: bad geometry", z)
    refused(lambda: kn.emb_fanin_bwd(None, d(g0), None, None, N, S, D, 0, lo, D + 1, z.t), "hulc_emb_fanin_bwd: bad geometry", z)


# ---- csrc/optim.hip: chunk sums, chunk gathers, casts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("W,chunk,dtype", [(1, 8, F32), (2, 1000, BF), (8, 8 * 4099, F32), (3, 8 * 131, BF), (2, 4096 * 256 * 4 + 8, BF)])
def test_sum_chunks(dev, W, chunk, dtype):
    """dst = sum over the W rank chunks in rank order, float32 accumulation; the last case is one vector past the grid cap (the stride loop)"""
    from hulc2_amd import kernels as kn

    g = _gen("chunks", W, chunk)
    src = rnd(_randn(g, W, chunk), dtype)
    dst = out_flat(dev, chunk, dtype)
    kn.sum_chunks(src.to(dtype).to(dev).reshape(-1), W, chunk, dst.t)
    torch.cuda.synchronize()
    dst.assert_guards("dst")
    f = src[0].float()
    for r in range(1, W):
        f = f + src[r].float()
    compare("sum_chunks", "dst", dst.value(), src.sum(0), f, MARGIN["SUM"], out_dtype=dtype)
    assert torch.equal(dst.value().cpu().reshape(-1), f.to(dtype)), "rank order, float32 accumulation, one rounding: the bits are determined"
    z = out_flat(dev, 16, dtype)
    refused(lambda: kn.sum_chunks(src.to(dtype).to(dev).reshape(-1), 1, 12, z.t), "hulc_sum_chunks: chunk must be a multiple of 8 elements, W >= 1", z)


@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_gather_chunks(dev, n):
    from hulc2_amd import kernels as kn

    g = _gen("gather", n)
    s0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (37, 2), generator=g, dtype=torch.int64).to(torch.int32)        # 8-byte chunks as raw bits
    s1 = torch.randint(-2 ** 31, 2 ** 31 - 1, (11, 2), generator=g, dtype=torch.int64).to(torch.int32)
    which = torch.rand(n, generator=g) < 0.3
    k = torch.where(which, torch.randint(0, 11, (n,), generator=g), torch.randint(0, 37, (n,), generator=g))
    idx = torch.where(which, k - 2 ** 31, k).to(torch.int32)                                                      # bit 31 selects the second source
    dst = Guarded(dev, n, 2, F32)
    kn.gather_chunks(s0.to(dev), s1.to(dev), dst.t, idx.to(dev))
    torch.cuda.synchronize()
    dst.assert_guards("dst")
    ref = torch.where(which[:, None], s1[k.clamp(max=10)], s0[k])
    assert torch.equal(dst.value().view(torch.int32).cpu(), ref)


def test_casts_are_bit_exact(dev):
    """float32 -> bf16 is round-to-nearest-even as torch's, including exact ties both ways, denormals, the overflow to infinity, signed zeros and
    infinities; NaN stays NaN.  bf16 -> float32 is the 16-bit shift.  Ragged counts take the scalar tail of both kernels."""
    from hulc2_amd import kernels as kn

    g = _gen("cast")
    special = torch.tensor([0x00000000, 0x80000000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF,     # ties, near-ties
                            0x00000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x80008000, 0x00800000,                                    # denormals
                            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000,                                    # overflow, infinities
                            0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F80FFFF], dtype=torch.int64)                             # NaNs
    rand_bits = torch.randint(0, 2 ** 32, (4099 - special.numel(),), generator=g, dtype=torch.int64)
    bits = torch.cat([special, rand_bits])
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    for n in (bits.numel(), 8, 3, 1):
        src = bits[:n].view(F32)
        dst = out_flat(dev, n, BF)
        kn.cast_f32_to_bf16(src.to(dev), dst.t, n)
        torch.cuda.synchronize()
        dst.assert_guards("bf16 dst")
        got, ref = dst.value().cpu().reshape(-1), src.to(BF)
        nan = torch.isnan(src)
        assert torch.equal(torch.isnan(got), nan), "NaN stays NaN, nothing else becomes one"
        assert torch.equal(got.view(torch.int16)[~nan], ref.view(torch.int16)[~nan]), "float32 -> bf16 differs from round-to-nearest-even"
    b16 = torch.randint(-2 ** 15, 2 ** 15, (4099,), generator=g, dtype=torch.int64).to(torch.int16)            # every kind of bf16 pattern, NaNs included
    for n in (4099, 16, 7, 1):
        dst = out_flat(dev, n, F32)
        kn.cast_bf16_to_f32(b16[:n].view(BF).to(dev), dst.t, n)
        torch.cuda.synchronize()
        dst.assert_guards("float32 dst")
        assert torch.equal(dst.value().view(torch.int32).cpu().reshape(-1), b16[:n].to(torch.int32) << 16)


# ------------------------------------------------------------------------------------------------
# unfused attention (S <= 32, head_dim 16)
# ------------------------------------------------------------------------------------------------
# B, S, H, spread of the scores
ATT = [
    (1, 1, 1, 1.0),         # one token: probability 1, out = v, dq = dk = 0
    (5, 7, 8, 1.0),         # ragged length, the model's head count
    (1, 16, 8, 1.0),        # the second half-wave entirely masked
    (5, 31, 1, 1.0),        # one key short of full
    (1, 32, 8, 1.0),        # the longest sequence the kernel takes
    (5, 32, 1, 60.0),       # scores spread over +-60: exp underflows for most keys
    (1, 17, 1, 60.0),       # one key in the second half-wave, spread scores
]


def _att_ref(qkv, dout, B, S, H, dt):
    E = H * 16
    q, k, v = (t.reshape(B, S, H, 16).permute(0, 2, 1, 3) for t in qkv.to(dt).reshape(B, S, 3, E).unbind(2))
    sc = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(16.0))
    p = torch.softmax(sc, -1)
    out = (p @ v).permute(0, 2, 1, 3).reshape(B * S, E)
    return p, out, (q, k, v)


def _att_ref_bwd(probs, qkv_split, dout, B, S, H, dt):
    q, k, v = qkv_split
    p = probs.to(dt)
    go = dout.to(dt).reshape(B, S, H, 16).permute(0, 2, 1, 3)
    dv = p.transpose(-1, -2) @ go
    dp = go @ v.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True)) * (1.0 / math.sqrt(16.0))
    dq, dk = ds @ k, ds.transpose(-1, -2) @ q
    return torch.stack([t.permute(0, 2, 1, 3).reshape(B * S, H * 16) for t in (dq, dk, dv)], 1).reshape(B * S, 3 * H * 16)


@pytest.mark.parametrize("B,S,H,spread", ATT)
def test_attention_fwd_bwd(dev, B, S, H, spread):
    from hulc2_amd import kernels as kn

    g = _gen("att", B, S, H, int(spread))
    E = H * 16
    qkv = _randn(g, B * S, 3 * E)
    scores = lambda t: (t[:, :E].reshape(B, S, H, 16).permute(0, 2, 1, 3) @ t[:, E:2 * E].reshape(B, S, H, 16).permute(0, 2, 3, 1)) / 4.0
    if spread > 1.0:
        qkv[:, :E] *= 60.0 / float(scores(qkv).abs().max())         # the largest score is +-60
    qkv = rnd(qkv, F32)
    out, probs = Guarded(dev, B * S, E), out_flat(dev, B * H * S * S)
    kn.attention_fwd(qkv.float().to(dev), out.t, probs.t, B, S, H, 16, 0.0, 0)
    torch.cuda.synchronize()
    out.assert_guards("out"); probs.assert_guards("probs")
    o1, p1 = out.value(), probs.value()
    rp, ro, split64 = _att_ref(qkv, None, B, S, H, torch.float64)
    fp, fo, _ = _att_ref(qkv, None, B, S, H, F32)
    if spread > 1.0:
        assert 59.0 < float(scores(qkv).abs().max()) < 61.0
    compare("attention_fwd", "probs", p1, rp, fp, MARGIN["FAST"])
    compare("attention_fwd", "out", o1, ro, fo, MARGIN["FAST"])
    out.t.fill_(float("nan")); probs.t.fill_(float("nan"))
    kn.attention_fwd(qkv.float().to(dev), out.t, probs.t, B, S, H, 16, 0.0, 0)
    torch.cuda.synchronize()
    same_bits(out.value(), o1, "attention_fwd out"); same_bits(probs.value(), p1, "attention_fwd probs")

    p32 = rnd(rp, F32)                                                # the saved probabilities, float32-rounded reference values
    dout = rnd(_randn(g, B * S, E), F32)
    dqkv = Guarded(dev, B * S, 3 * E)
    args = (qkv.float().to(dev), p32.float().to(dev).reshape(-1), dout.float().to(dev), dqkv.t, B, S, H, 16, 0.0, 0)
    kn.attention_bwd(*args)
    torch.cuda.synchronize()
    dqkv.assert_guards("dqkv")
    d1 = dqkv.value()
    r = _att_ref_bwd(p32, split64, dout, B, S, H, torch.float64)
    f = _att_ref_bwd(p32, tuple(t.float() for t in split64), dout, B, S, H, F32)
    compare("attention_bwd", "dqkv", d1, r, f, MARGIN["FAST"], grad=True)
    dqkv.t.fill_(float("nan"))
    kn.attention_bwd(*args)
    torch.cuda.synchronize()
    same_bits(dqkv.value(), d1, "attention_bwd dqkv")


def test_attention_refuses_what_it_cannot_run(dev):
    from hulc2_amd import kernels as kn

    B, S, H = 1, 33, 1
    qkv = torch.ones(B * S, 48, device=dev)
    out, probs, dqkv = Guarded(dev, B * S, 16), out_flat(dev, B * H * S * S), Guarded(dev, B * S, 48)
    refused(lambda: kn.attention_fwd(qkv, out.t, probs.t, B, S, H, 16, 0.0, 0), "hulc_attention_fwd: needs S <= 32 and head_dim == 16", out, probs)
    refused(lambda: kn.attention_bwd(qkv, torch.ones(S * S, device=dev), torch.ones(B * S, 16, device=dev), dqkv.t, B, S, H, 16, 0.0, 0),
            "hulc_attention_bwd: needs S <= 32 and head_dim == 16", dqkv)
    refused(lambda: kn.attention_fwd(qkv, out.t, probs.t, B, 8, H, 32, 0.0, 0), "hulc_attention_fwd: needs S <= 32 and head_dim == 16", out, probs)
