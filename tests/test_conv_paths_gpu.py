"""Kernel-level tests of the conv family (csrc/conv.hip, conv_band.hip, conv_band_planes.hip, conv1_band.hip, conv_wgrad_band.hip) through the four
entry points hulc_conv2d_fwd / hulc_conv2d_padded_fwd / hulc_conv2d_bwd_data / hulc_conv2d_bwd_weight, every kernel instance against torch's
convolution in float64.  The pattern of a case and the tolerance rule are in tests/kcheck.py; what is particular to this file:

LATTICE cases.  Operands are bf16 and the accumulators fp32, so on a small dyadic lattice — x, dy and the activations integers in [-3, 3] (masks:
relu of such integers), w integers in [-3, 3] / 8, bias and the accumulate bases of dW / db multiples of 1/8 in [-2, 2] — every partial sum is
an integer multiple of 1/8 below 2^24 / 8 and therefore exact in fp32 WHATEVER the summation order.  A correct kernel equals the float64 convolution
bit for bit (`torch.equal`; a bf16 / fp16 output equals the reference rounded once).  A dropped tap, a wrong parity class, a stale band or a
mis-clipped ragged unit cannot hide behind rounding.  Each case asserts the 2^24 precondition from the float64 reference's own max-abs.

RANDOM cases, one per kernel token at the token's smallest shape: seeded float64 values rounded to the storage type, `compare()` against the
float64 reference with torch's CPU float32 convolution of the same operands as the yardstick, plus the flat bounds tests/test_conv_gpu.py uses
for the same operation (forward 2e-4, data gradient 5e-4, dW 1e-4 * scale + 1e-4, db 1e-4 * scale + 1e-3).

PATH.  Every case states the kernel token and the plan (R / F / units / grid) it means to hit and asserts them against kernels.conv_last_path()
after the call: the expectations replay the launchers' host arithmetic, so an edit of a threshold (the 128- or 96-pixel cut, an LDS budget) fails
here instead of silently turning a band test into a gather test.  units / grid > 1 means a persistent walk of that many units per workgroup.

Outputs (y, y_bf16, dx, dw, db, planes) live inside sentinel-filled allocations whose guard bands must survive the call; inputs live inside
NaN-sentinel allocations, so a read past a frame, a band or a ragged last unit that is consumed surfaces as a non-finite output."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import kcheck as K
from tests.kcheck import compare, out_flat, refused, rnd, same_bits

pytestmark = pytest.mark.gpu

# Margins of margin * max(e_ref, 2^-23), e_ref = torch's CPU float32 convolution against float64 (tests/kcheck.py).
#   SUM 4: the class of tests/test_reductions_gpu.py — products of bf16 operands are exact in fp32, so only the order of the fp32 sums differs
#          from the CPU's.
# A token that cannot meet 4 is a finding and gets a row here with the measured float32-CPU and GPU errors and the cause; its margin is then at
# most the project's other class (16).
#   token                         what     cpu-f32     gpu        cause
#   (none)
MARGIN = {"SUM": 4.0}

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32

# name -> (Cin, Cout, K, stride, x_nchw): the three layers of both camera encoders
GEOM = {"conv1": (3, 32, 8, 4, True), "conv2": (32, 64, 4, 2, False), "conv3": (64, 64, 3, 1, False)}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    K.report("tests/test_conv_paths_gpu.py")


def _gen(*key):
    seed = 0
    for k in key:
        for ch in (k if isinstance(k, str) else repr(k)):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _uni(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


def _in(dev, t64, dtype, lead=0):
    """an input tensor inside a NaN-sentinel allocation (`lead` elements in: a view that is not 16-byte aligned)"""
    return out_flat(dev, t64.numel(), dtype, init=t64, lead=lead).t.reshape(t64.shape)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _pack_bits(pos_nhwc):
    """reference sign planes of a boolean NHWC map: (C / 32, npix) int32 flattened, bit c % 32 of plane c / 32"""
    C = pos_nhwc.shape[-1]
    w = (pos_nhwc.reshape(-1, C // 32, 32).to(torch.int64) << torch.arange(32, device=pos_nhwc.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).t().contiguous().reshape(-1)


def _plan(text):
    words = text.split()
    plan = {}
    for w in words[1:]:
        if w.startswith("+"):
            plan[w[1:]] = 1
        else:
            k, v = w.split("=")
            plan[k] = int(v)
    return words[0], plan


def _assert_path(expect, what):
    """the kernel token and the launcher's plan of the call just made; registers the token for the module's [kcheck-max] table"""
    from hulc2_amd import kernels as kn

    got = kn.conv_last_path()
    assert got == _plan(expect), f"{what}: served by {got}, the case means to hit {_plan(expect)}"
    K.RATIOS.setdefault(_name(expect), 0.0)


def _name(expect):
    """the row of the [kcheck-max] table: the token and the fields that select a kernel instance"""
    tok, plan = _plan(expect)
    return " ".join([tok] + [f"{k}={plan[k]}" for k in ("xf32", "bits", "multi", "pad", "u8", "x3", "pure16", "f32") if k in plan])


def _exact_lattice(ref64, what, extra=0.0):
    top = (ref64.abs().max().item() + extra) * 8
    assert top < 2 ** 24, f"{what}: the largest sum is {top:.0f} units of 2^-3, not below 2^24: the lattice is no longer exact in fp32"


def _lattice_equal(got, ref64, dtype, what):
    want = ref64.float().to(dtype)                       # (the exact value fits fp32: one rounding to a low-precision output)
    assert got.dtype == dtype and torch.equal(got, want), (
        f"{what}: {(got != want).sum().item()} of {got.numel()} elements differ from the float64 convolution "
        f"(max abs difference {(got.double() - want.double()).abs().max().item():.3e}, non-finite {(~torch.isfinite(got.float())).sum().item()})")


def _flat(got, ref64, dtype, bound, what):
    err = ((got.double() - ref64).abs() - K.half_ulp(ref64, dtype)).clamp_min(0).max().item()
    assert err < bound, f"{what}: max abs error {err:.3e} (flat bound {bound:g}, reference max {ref64.abs().max().item():.3e})"


# ------------------------------------------------------------------------------------------------
# forward (hulc_conv2d_fwd, hulc_conv2d_padded_fwd)
# ------------------------------------------------------------------------------------------------
def _fwd(dev, geom, N, H, W, mode, expect, xdt=BF, ydt=BF, wdt=BF, bits=False, y16=False, lead=0, compute=None, pad=None, add=False, w_lo=False,
         relu=True):
    from hulc2_amd import kernels as kn

    Cin, Cout, Kk, s, nchw = geom
    what = f"fwd {geom} {(N, H, W)} {mode} -> {expect}"
    cmode = kn.BF16 if compute is None else compute
    g = _gen("fwd", geom, N, H, W, mode, str(xdt), str(ydt), bits, y16, lead, pad)
    p = 0 if pad is None else pad
    OH, OW = (H + 2 * p - Kk) // s + 1, (W + 2 * p - Kk) // s + 1
    a64 = None
    if mode == "lattice":
        x64, w64, b64 = _ints(g, N, Cin, H, W), _ints(g, Cout, Cin, Kk, Kk) / 8, _ints(g, Cout, lo=-16, hi=16) / 8
        if add:
            a64 = _ints(g, N, Cout, OH, OW)
    else:
        x64, w64 = rnd(_uni(g, N, Cin, H, W), xdt), rnd(_uni(g, Cout, Cin, Kk, Kk) / (Cin * Kk * Kk) ** 0.5, wdt if not w_lo else F32)
        b64 = rnd(_uni(g, Cout) * 0.1, F32)
        if xdt == F32 and compute is None and not w_lo:  # (fp32 activations of a bf16 step are rounded while staged: the reference gets what is multiplied)
            x64 = rnd(x64, BF)
        if add:
            a64 = rnd(_uni(g, N, Cout, OH, OW), ydt)
    lay = (lambda t: t.contiguous()) if nchw else _nhwc
    wl = (lambda t: t.reshape(Cout, -1).contiguous()) if nchw else (lambda t: _nhwc(t).reshape(Cout, -1))
    x = _in(dev, lay(x64), xdt, lead)
    wlo = None
    if w_lo:                                             # hi + lo bf16 splits of both operands: the kernel multiplies hi hi + hi lo + lo hi
        whi64 = rnd(w64, BF)
        wlo64 = rnd(w64 - whi64, BF)
        xhi64 = rnd(x64, BF)
        xlo64 = rnd(x64 - xhi64, BF)
        w2d, wlo = _in(dev, wl(whi64), BF), _in(dev, wl(wlo64), BF)
    else:
        w2d = _in(dev, wl(w64), wdt)
    b = _in(dev, b64, F32)
    a = _in(dev, _nhwc(a64), ydt) if add else None

    def ref(dt, where):
        c = lambda xx, ww: F.conv2d(xx.to(where, dt), ww.to(where, dt), None, stride=s, padding=p)
        z = (c(xhi64, whi64) + c(xhi64, wlo64) + c(xlo64, whi64)) if w_lo else c(x64, w64)
        z = z + b64.to(where, dt)[None, :, None, None]
        if add:
            z = z + a64.to(where, dt)
        return _nhwc(z)

    z64 = ref(torch.float64, dev)
    r64 = torch.relu(z64) if relu else z64

    def call():
        n = N * OH * OW * Cout
        y = out_flat(dev, n, ydt)
        yb = out_flat(dev, n, BF) if y16 else None
        pl = out_flat(dev, n // 32, torch.int32) if bits else None
        yv = y.t.reshape(N, OH, OW, Cout)
        if pad is None:
            kn.conv2d_fwd(x, w2d, b, yv, N, H, W, Cin, Cout, Kk, Kk, s, nchw, relu=relu, compute=cmode, relu_bits=pl.t.reshape(-1) if bits else None,
                          w_lo=wlo, y_bf16=yb.t.reshape(N, OH, OW, Cout) if y16 else None)
        else:
            kn.conv2d_padded_fwd(x, w2d, b, yv, N, H, W, Cin, Cout, Kk, Kk, s, pad, relu=relu, add=a, compute=cmode)
        _assert_path(expect, what)
        torch.cuda.synchronize()
        for o, nm in ((y, "y"), (yb, "y_bf16"), (pl, "planes")):
            if o is not None:
                o.assert_guards(f"{what} {nm}")
        return y.value().reshape(N, OH, OW, Cout), yb.value().reshape(N, OH, OW, Cout) if y16 else None, pl.value().reshape(-1) if bits else None

    y, yb, pl = call()
    if relu:
        frac = (r64 > 0).double().mean().item()
        assert 0.2 < frac < 0.8, f"{what}: {frac:.2f} of the outputs are positive, the ReLU means nothing"
    if mode == "lattice":
        _exact_lattice(z64, what)
        _lattice_equal(y, r64, ydt, what + " y")
        if y16:
            _lattice_equal(yb, r64, BF, what + " y_bf16")
        if bits:
            want = _pack_bits(r64 > 0)
            assert torch.equal(pl, want), f"{what}: {(pl != want).sum().item()} of {pl.numel()} sign words differ from the packed (ref > 0)"
    else:
        r32 = ref(torch.float32, "cpu")
        r32 = torch.relu(r32) if relu else r32
        compare(_name(expect), "y", y, r64, r32, MARGIN["SUM"], out_dtype=ydt)
        _flat(y, r64, ydt, 2e-4, what + " y")
        if y16:
            compare(_name(expect), "y_bf16", yb, r64, r32, MARGIN["SUM"], out_dtype=BF)
        if bits:                                         # (a value within rounding of zero may take either sign: the planes describe the STORED map)
            assert torch.equal(pl, _pack_bits(y > 0)), f"{what}: the planes differ from the stored map's signs"
    y2, yb2, pl2 = call()
    same_bits(y, y2, what + " y")
    if y16:
        same_bits(yb, yb2, what + " y_bf16")
    if bits:
        same_bits(pl, pl2, what + " planes")


BX2 = "band_x<32,2,4,4,2> xf32=0 "
BX3 = "band_x<64,2,3,3,1> xf32=0 bits=0 "
# conv2 forward: (N, H, W), the plan behind "band_x<32,2,4,4,2> xf32=0 bits=B " or the whole path
FWD2_BAND = [
    ((2, 20, 20), "multi=1 R=9 F=2 units=1 grid=1"),       # packed frames, one unit; (1, 20, 20) below is the other side of the 128-pixel cut
    ((5, 20, 20), "multi=1 R=9 F=3 units=2 grid=2"),       # ragged last unit of 2 frames
    ((1, 36, 36), "multi=0 R=17 F=1 units=1 grid=1"),      # one whole frame
    ((3, 49, 49), "multi=0 R=12 F=1 units=6 grid=6"),      # two bands per frame, R = 12 of OH = 23: unequal last band
]


@pytest.mark.parametrize("ydt,bits", [(BF, False), (BF, True), (F32, False), (F32, True)], ids=["bf16", "bf16+planes", "f32", "f32+planes"])
@pytest.mark.parametrize("shape,plan", FWD2_BAND, ids=[str(s) for s, _ in FWD2_BAND])
def test_conv2_forward_band_lattice(dev, shape, plan, ydt, bits):
    """the planes ride in the band kernel's epilogue next to a bf16 output; next to an fp32 output they come from the second pass"""
    in_kernel = bits and ydt == BF
    _fwd(dev, GEOM["conv2"], *shape, "lattice", BX2 + f"bits={int(in_kernel)} " + plan + (" +relu_bits_pass" if bits and not in_kernel else ""),
         ydt=ydt, bits=bits)


@pytest.mark.parametrize("shape,expect,bits", [
    ((1, 20, 20), "gather<bf16>", False),                                                     # 81 pixels in the only unit: under the 128-pixel cut
    ((2, 17, 21), "gather<bf16> +relu_bits_pass", True),                                      # 2 x 7 x 9 = 126 pixels
    ((130, 49, 49), BX2 + "bits=1 multi=0 R=12 F=1 units=260 grid=130", True),                # 2 units per workgroup
    ((771, 20, 20), BX2 + "bits=1 multi=1 R=9 F=3 units=257 grid=129", True),                 # packed units, 2 per workgroup, one workgroup gets 1
], ids=["1x20x20", "2x17x21", "130x49x49", "771x20x20"])
def test_conv2_forward_gather_and_persistent_lattice(dev, shape, expect, bits):
    _fwd(dev, GEOM["conv2"], *shape, "lattice", expect, bits=bits)


def test_conv2_forward_fp32_frames_lattice(dev):
    """the xf32 instance: fp32 activations converted while the band is staged, bf16 weights, fp32 output"""
    _fwd(dev, GEOM["conv2"], 2, 20, 20, "lattice", "band_x<32,2,4,4,2> xf32=1 bits=0 multi=1 R=9 F=2 units=1 grid=1", xdt=F32, ydt=F32)


FWD3 = [
    # shape, path, y type, y_bf16 twin
    ((3, 23, 23), "band_planes<23,23> bits=0 units=3 grid=3", BF, False),
    ((3, 23, 23), "band_planes<23,23> bits=0 units=3 grid=3", F32, True),
    ((3, 23, 23), "band_planes<23,23> bits=0 units=3 grid=3", F16, True),
    ((520, 23, 23), "band_planes<23,23> bits=0 units=520 grid=174", BF, False),               # 3 units per workgroup, the last two workgroups short
    ((1, 20, 20), "band_glds<2,3,3> bits=0 pad=0 units=1 grid=1", BF, False),                  # the instance only these shapes reach
    ((1, 24, 22), "band_glds<2,3,3> bits=0 pad=0 units=1 grid=1", BF, False),
    ((520, 20, 20), "band_glds<2,3,3> bits=0 pad=0 units=520 grid=174", BF, False),            # A / B band alternation, the outer loop's second pass
    ((2, 9, 9), "gather<bf16>", BF, False),                                                    # 98 pixels: under the cut
    ((3, 9, 9), BX3 + "multi=1 R=7 F=3 units=1 grid=1", BF, False),
    ((11, 9, 9), BX3 + "multi=1 R=7 F=7 units=2 grid=2", BF, False),                           # ragged: 7 + 4 frames
    ((1, 40, 40), BX3 + "multi=0 R=13 F=1 units=3 grid=3", BF, False),                         # the frame fits neither direct-to-LDS band
    ((2, 11, 13), BX3 + "multi=1 R=9 F=2 units=1 grid=1", F32, True),                          # the band kernel's own twin store
    ((1, 9, 9), "gather<bf16> +cast_pass", F32, True),
]


@pytest.mark.parametrize("shape,expect,ydt,y16", FWD3, ids=[f"{s}-{str(t).split('.')[-1]}" for s, _, t, _ in FWD3])
def test_conv3_forward_lattice(dev, shape, expect, ydt, y16):
    _fwd(dev, GEOM["conv3"], *shape, "lattice", expect, ydt=ydt, y16=y16)


C1 = "conv1_band u8=0 "
FWD1 = [
    ((3, 44, 44), C1 + "x3=0 R=10 grid=3"),                # whole-frame unit
    ((5, 84, 84), C1 + "x3=0 R=10 grid=5"),                # two bands
    ((3, 200, 200), C1 + "x3=0 R=4 grid=3"),
    ((3, 86, 84), "gather<bf16>"),                         # (H - 8) % 4 != 0: rows the stride never reaches, the band kernel declines
    ((4, 36, 36), C1 + "x3=0 R=8 grid=4"),
]


@pytest.mark.parametrize("shape,expect", FWD1, ids=[str(s) for s, _ in FWD1])
def test_conv1_forward_lattice(dev, shape, expect):
    _fwd(dev, GEOM["conv1"], *shape, "lattice", expect, xdt=F32, ydt=BF, bits=expect.startswith("conv1_band"))


R18 = (64, 64, 3, 1, False)
PADDED = [
    (R18, (1, 56, 56), 1, BX3 + "multi=0 R=8 F=1 units=7 grid=7"),                             # zero rows only at the first and the last band
    (R18, (3, 14, 14), 1, BX3 + "multi=1 R=14 F=2 units=2 grid=2"),                            # packed, ragged
    (R18, (2, 7, 7), 1, "gather<bf16>"),                                                       # 98 pixels: gather with bounds checks
    ((64, 128, 3, 2, False), (2, 14, 14), 1, "gather<bf16>"),
    ((64, 128, 1, 2, False), (2, 28, 28), 0, "gather<bf16>"),
]


@pytest.mark.parametrize("geom,shape,pad,expect", PADDED, ids=[f"{g[1]}c-{g[2]}x{g[2]}s{g[3]}-{s}" for g, s, _, _ in PADDED])
def test_padded_forward_lattice(dev, geom, shape, pad, expect):
    _fwd(dev, geom, *shape, "lattice", expect, pad=pad, add=True)


FWD_RANDOM = [
    # one per kernel instance, at its smallest shape of the tables above
    ("conv2", (2, 20, 20), BX2 + "bits=1 multi=1 R=9 F=2 units=1 grid=1", dict(bits=True)),
    ("conv2", (1, 36, 36), BX2 + "bits=0 multi=0 R=17 F=1 units=1 grid=1", dict(ydt=F32)),
    ("conv2", (2, 20, 20), "band_x<32,2,4,4,2> xf32=1 bits=0 multi=1 R=9 F=2 units=1 grid=1", dict(xdt=F32, ydt=F32)),
    ("conv2", (1, 20, 20), "gather<bf16>", dict(ydt=F32)),
    ("conv3", (3, 23, 23), "band_planes<23,23> bits=0 units=3 grid=3", dict(ydt=F16, y16=True)),
    ("conv3", (1, 20, 20), "band_glds<2,3,3> bits=0 pad=0 units=1 grid=1", dict()),
    ("conv3", (3, 9, 9), BX3 + "multi=1 R=7 F=3 units=1 grid=1", dict(ydt=F32, y16=True)),
    ("conv3", (1, 40, 40), BX3 + "multi=0 R=13 F=1 units=3 grid=3", dict()),
    ("conv1", (3, 44, 44), C1 + "x3=0 R=10 grid=3", dict(xdt=F32, ydt=F32)),
    ("conv1", (3, 44, 44), C1 + "x3=1 R=10 grid=3", dict(xdt=F32, ydt=F32, w_lo=True)),
    ("conv1", (3, 86, 84), "gather<bf16>", dict(xdt=F32, ydt=F32)),
]


@pytest.mark.parametrize("layer,shape,expect,kw", FWD_RANDOM, ids=[f"{l}-{s}-{_name(e)}" for l, s, e, _ in FWD_RANDOM])
def test_forward_random(dev, layer, shape, expect, kw):
    _fwd(dev, GEOM[layer], *shape, "random", expect, **kw)


def test_padded_forward_random(dev):
    _fwd(dev, R18, 3, 14, 14, "random", BX3 + "multi=1 R=14 F=2 units=2 grid=2", pad=1, add=True)
    _fwd(dev, R18, 2, 7, 7, "random", "gather<bf16>", pad=1, add=True)


# ------------------------------------------------------------------------------------------------
# data gradient (hulc_conv2d_bwd_data)
# ------------------------------------------------------------------------------------------------
def _dgrad(dev, geom, N, H, W, mode, expect, mask="tensor", dt=BF, wdt=BF, lead=0, compute=None):
    """dx over the layer input (N, H, W, Cin); mask: "planes" (the sign planes of the layer input next to the tensor, as the model passes them),
    "tensor" (the activation only) or None"""
    from hulc2_amd import kernels as kn

    Cin, Cout, Kk, s, _ = geom
    what = f"dgrad {geom} {(N, H, W)} {mode} mask={mask} -> {expect}"
    cmode = kn.BF16 if compute is None else compute
    g = _gen("dgrad", geom, N, H, W, mode, mask, str(dt), lead)
    OH, OW = (H - Kk) // s + 1, (W - Kk) // s + 1
    if mode == "lattice":
        dy64, w64, act64 = _ints(g, N, Cout, OH, OW), _ints(g, Cout, Cin, Kk, Kk) / 8, torch.relu(_ints(g, N, Cin, H, W))
    else:
        dy64 = rnd(torch.randn(N, Cout, OH, OW, generator=g, dtype=torch.float64), dt)
        w64 = rnd(_uni(g, Cout, Cin, Kk, Kk) / (Cin * Kk * Kk) ** 0.5, wdt)
        act64 = rnd(torch.relu(torch.randn(N, Cin, H, W, generator=g, dtype=torch.float64)), dt)
        if dt == F32 and compute is None:                # (an fp32 gradient map of a bf16 step is rounded while staged)
            dy64 = rnd(dy64, BF)
    dy = _in(dev, _nhwc(dy64), dt, lead)
    wt = _in(dev, w64.permute(1, 2, 3, 0).contiguous(), wdt)                 # [Cin][KH][KW][Cout]
    act = _in(dev, _nhwc(act64), dt) if mask else None
    planes = _in(dev, _pack_bits(_nhwc(act64) > 0).double(), torch.int32) if mask == "planes" else None

    def ref(dtp, where):
        r = torch.nn.grad.conv2d_input((N, Cin, H, W), w64.to(where, dtp), dy64.to(where, dtp), stride=s)
        return _nhwc(r * (act64.to(where) > 0) if mask else r)

    r64 = ref(torch.float64, dev)

    def call():
        dx = out_flat(dev, N * H * W * Cin, dt)                              # (sentinel-filled: an uncovered pixel shows)
        kn.conv2d_bwd_data(dy, wt, dx.t.reshape(N, H, W, Cin), act, N, H, W, Cin, Cout, Kk, Kk, s, compute=cmode, relu_bits=planes)
        _assert_path(expect, what)
        torch.cuda.synchronize()
        dx.assert_guards(what + " dx")
        return dx.value().reshape(N, H, W, Cin)

    dx = call()
    if mask:
        frac = (act64 > 0).double().mean().item()
        assert 0.2 < frac < 0.8, f"{what}: {frac:.2f} of the mask is set, the mask means nothing"
    if mode == "lattice":
        _exact_lattice(r64, what)
        _lattice_equal(dx, r64, dt, what + " dx")
    else:
        compare(_name(expect), "dx", dx, r64, ref(torch.float32, "cpu"), MARGIN["SUM"], out_dtype=dt)
        _flat(dx, r64, dt, 5e-4, what + " dx")
    same_bits(dx, call(), what + " dx")


GL4 = "band_glds<4,2,2> bits=2 pad=1 "
BXD2 = "band_x<64,4,2,2,1> "
DG2 = [
    ((3, 49, 49), "planes", GL4 + "units=3 grid=3", BF),                                       # odd H, W: parity classes of 25 and 24
    ((1, 32, 32), "planes", GL4 + "units=1 grid=1", BF),                                       # even sizes
    ((520, 32, 32), "planes", GL4 + "units=520 grid=174", BF),                                 # 3 units per workgroup
    ((3, 49, 49), "tensor", BXD2 + "xf32=0 bits=0 multi=0 R=25 F=1 units=3 grid=3", BF),
    ((1, 31, 33), "tensor", BXD2 + "xf32=0 bits=0 multi=0 R=16 F=1 units=1 grid=1", BF),
    ((5, 20, 20), "tensor", BXD2 + "xf32=0 bits=0 multi=1 R=10 F=5 units=1 grid=1", BF),
    ((5, 20, 20), "planes", BXD2 + "xf32=0 bits=2 multi=1 R=10 F=5 units=1 grid=1", BF),       # too few pixels for the direct-to-LDS instance
    ((2, 17, 21), "tensor", BXD2 + "xf32=0 bits=0 multi=1 R=9 F=2 units=1 grid=1", BF),
    ((1, 20, 20), "tensor", "gather<bf16> launches=4", BF),                                    # 100 pixels: under the cut, one launch per parity class
    ((3, 49, 49), None, BXD2 + "xf32=0 bits=0 multi=0 R=25 F=1 units=3 grid=3", BF),           # no mask at all
    ((2, 20, 20), None, BXD2 + "xf32=1 bits=0 multi=1 R=10 F=2 units=1 grid=1", F32),          # fp32 dy / dx, bf16 weights
]


@pytest.mark.parametrize("shape,mask,expect,dt", DG2, ids=[f"{s}-{m}-{str(t).split('.')[-1]}" for s, m, _, t in DG2])
def test_conv2_data_gradient_lattice(dev, shape, mask, expect, dt):
    _dgrad(dev, GEOM["conv2"], *shape, "lattice", expect, mask=mask, dt=dt)


BXD3 = "band_x<64,2,3,3,1> xf32=0 "
DG3 = [
    ((3, 23, 23), "planes", "band_planes<21,21> bits=2 units=3 grid=3"),
    ((520, 23, 23), "planes", "band_planes<21,21> bits=2 units=520 grid=174"),
    ((1, 22, 22), "planes", "band_glds<2,3,3> bits=2 pad=1 units=1 grid=1"),                   # the instance only these shapes reach
    ((1, 22, 20), "planes", "band_glds<2,3,3> bits=2 pad=1 units=1 grid=1"),
    ((1, 24, 24), "tensor", BXD3 + "bits=0 multi=0 R=12 F=1 units=2 grid=2"),                  # taps cross a band edge into real rows, not zeros
    ((5, 9, 9), "tensor", BXD3 + "bits=0 multi=1 R=9 F=5 units=1 grid=1"),
    ((2, 11, 13), "planes", BXD3 + "bits=2 multi=1 R=11 F=2 units=1 grid=1"),
]


@pytest.mark.parametrize("shape,mask,expect", DG3, ids=[f"{s}-{m}" for s, m, _ in DG3])
def test_conv3_data_gradient_lattice(dev, shape, mask, expect):
    _dgrad(dev, GEOM["conv3"], *shape, "lattice", expect, mask=mask)


DG_RANDOM = [
    ("conv2", (1, 32, 32), "planes", GL4 + "units=1 grid=1", BF),
    ("conv2", (1, 31, 33), "tensor", BXD2 + "xf32=0 bits=0 multi=0 R=16 F=1 units=1 grid=1", BF),
    ("conv2", (2, 17, 21), "tensor", BXD2 + "xf32=0 bits=0 multi=1 R=9 F=2 units=1 grid=1", BF),
    ("conv2", (5, 20, 20), "planes", BXD2 + "xf32=0 bits=2 multi=1 R=10 F=5 units=1 grid=1", BF),
    ("conv2", (2, 20, 20), None, BXD2 + "xf32=1 bits=0 multi=1 R=10 F=2 units=1 grid=1", F32),
    ("conv2", (1, 20, 20), "tensor", "gather<bf16> launches=4", BF),
    ("conv3", (3, 23, 23), "planes", "band_planes<21,21> bits=2 units=3 grid=3", BF),
    ("conv3", (1, 22, 20), "planes", "band_glds<2,3,3> bits=2 pad=1 units=1 grid=1", BF),
    ("conv3", (1, 24, 24), "tensor", BXD3 + "bits=0 multi=0 R=12 F=1 units=2 grid=2", BF),
    ("conv3", (2, 11, 13), "planes", BXD3 + "bits=2 multi=1 R=11 F=2 units=1 grid=1", BF),
]


@pytest.mark.parametrize("layer,shape,mask,expect,dt", DG_RANDOM, ids=[f"{l}-{s}-{_name(e)}" for l, s, _, e, _ in DG_RANDOM])
def test_data_gradient_random(dev, layer, shape, mask, expect, dt):
    _dgrad(dev, GEOM[layer], *shape, "random", expect, mask=mask, dt=dt)


# ------------------------------------------------------------------------------------------------
# weight gradient (hulc_conv2d_bwd_weight)
# ------------------------------------------------------------------------------------------------
def _wgrad(dev, geom, N, H, W, mode, expect, xdt=BF, dydt=BF, lead=0, compute=None):
    """dW + db three ways: plain (the forward k order), dw_oihw=True, and dw_oihw + accumulate onto a base"""
    from hulc2_amd import kernels as kn

    Cin, Cout, Kk, s, nchw = geom
    what = f"wgrad {geom} {(N, H, W)} {mode} -> {expect}"
    cmode = kn.BF16 if compute is None else compute
    g = _gen("wgrad", geom, N, H, W, mode, str(xdt), str(dydt), lead)
    OH, OW = (H - Kk) // s + 1, (W - Kk) // s + 1
    Kd = Cin * Kk * Kk
    if mode == "lattice":
        x64, dy64 = _ints(g, N, Cin, H, W), _ints(g, N, Cout, OH, OW)
        bw64, bb64 = _ints(g, Cout, Kd, lo=-16, hi=16) / 8, _ints(g, Cout, lo=-16, hi=16) / 8
    else:
        x64 = rnd(_uni(g, N, Cin, H, W), xdt)
        dy64 = rnd(torch.randn(N, Cout, OH, OW, generator=g, dtype=torch.float64), dydt)
        if compute is None and xdt == F32:               # (fp32 operands of a bf16 step are rounded by the kernel: the reference gets what it multiplies)
            x64 = rnd(x64, BF)
        if compute is None and dydt == F32:
            dy64 = rnd(dy64, BF)
        bw64, bb64 = rnd(torch.randn(Cout, Kd, generator=g, dtype=torch.float64), F32), rnd(torch.randn(Cout, generator=g, dtype=torch.float64), F32)
    x = _in(dev, x64.contiguous() if nchw else _nhwc(x64), xdt, lead)
    dy = _in(dev, _nhwc(dy64), dydt)

    def ref(dt, where):
        r = torch.nn.grad.conv2d_weight(x64.to(where, dt), (Cout, Cin, Kk, Kk), dy64.to(where, dt), stride=s)
        return r, dy64.to(where, dt).sum(dim=(0, 2, 3))

    rw64, rb64 = ref(torch.float64, dev)
    k_order = (lambda r: r.reshape(Cout, -1)) if nchw else (lambda r: _nhwc(r).reshape(Cout, -1))
    oihw = lambda r: r.reshape(Cout, -1)

    def call(dw_oihw, accumulate):
        dw = out_flat(dev, Cout * Kd, F32, init=bw64 if accumulate else None)
        db = out_flat(dev, Cout, F32, init=bb64 if accumulate else None)
        kn.conv2d_bwd_weight(x, dy, dw.t.reshape(Cout, Kd), db.t.reshape(Cout), N, H, W, Cin, Cout, Kk, Kk, s, nchw, compute=cmode,
                             dw_oihw=dw_oihw, accumulate=accumulate)
        _assert_path(expect, what)
        torch.cuda.synchronize()
        dw.assert_guards(what + " dw")
        db.assert_guards(what + " db")
        return dw.value().reshape(Cout, Kd), db.value().reshape(Cout)

    if mode == "lattice":
        _exact_lattice(rw64, what + " dW", extra=2.0)
        _exact_lattice(rb64, what + " db", extra=2.0)
    else:
        rw32, rb32 = ref(torch.float32, "cpu")
    for dw_oihw, accumulate in ((False, False), (True, False), (True, True)):
        tag = f"{what} ({'OIHW' if dw_oihw else 'k order'}{', accumulated' if accumulate else ''})"
        order = oihw if dw_oihw else k_order
        dw, db = call(dw_oihw, accumulate)
        ww, wb = order(rw64) + (bw64.to(dev) if accumulate else 0), rb64 + (bb64.to(dev) if accumulate else 0)
        if mode == "lattice":
            _lattice_equal(dw, ww, F32, tag + " dW")
            _lattice_equal(db, wb, F32, tag + " db")
        else:
            w32, b32 = order(rw32) + (bw64.float() if accumulate else 0), rb32 + (bb64.float() if accumulate else 0)
            compare(_name(expect), "dW", dw, ww, w32, MARGIN["SUM"], grad=True)
            compare(_name(expect), "db", db, wb, b32, MARGIN["SUM"], grad=True)
            _flat(dw, ww, F32, 1e-4 * rw64.abs().max().item() + 1e-4, tag + " dW")
            _flat(db, wb, F32, 1e-4 * rb64.abs().max().item() + 1e-3, tag + " db")
        if not dw_oihw:
            dw2, db2 = call(dw_oihw, accumulate)
            same_bits(dw, dw2, tag + " dW")
            same_bits(db, db2, tag + " db")


WB3 = "wband<64,2,3,3,1> "
WG3 = [
    ((1, 9, 9), "wgrad_gather f32=0 P=1", (True, False)),                  # 49 pixels: under the 96-pixel cut
    ((2, 9, 9), "R=7 F=2 units=1 grid=1", (True, False)),                  # 98 pixels: over it
    ((5, 9, 9), "R=7 F=3 units=2 grid=2", (True, False)),                  # ragged
    ((1, 12, 12), "R=10 F=1 units=1 grid=1", (True, False)),
    ((1, 30, 30), "R=7 F=1 units=4 grid=4", (True,)),                      # 4 bands of 7
    ((3, 23, 23), "R=11 F=1 units=6 grid=6", (True,)),
    ((300, 23, 23), "R=11 F=1 units=600 grid=200", (True,)),               # 3 units per workgroup
    ((520, 12, 12), "R=10 F=2 units=260 grid=130", (True,)),               # 2 packed units per workgroup
]
WB2 = "wband<32,2,4,4,2> "
WG2 = [
    ((2, 20, 20), "R=9 F=2 units=1 grid=1", (True, False)),
    ((5, 20, 20), "R=9 F=3 units=2 grid=2", (True, False)),
    ((2, 17, 21), "R=7 F=2 units=1 grid=1", (True, False)),
    ((1, 24, 24), "R=11 F=1 units=1 grid=1", (True,)),
    ((3, 49, 49), "R=12 F=1 units=6 grid=6", (True,)),
    ((300, 49, 49), "R=12 F=1 units=600 grid=200", (True,)),
]


def _wg_cases(table, token):
    for shape, plan, pures in table:
        for pure in pures:
            yield pytest.param(shape, plan if plan.startswith("wgrad_gather") else f"{token}pure16={int(pure)} {plan}", pure,
                               id=f"{shape}-{'bf16' if pure else 'f32'}")


@pytest.mark.parametrize("shape,expect,pure16", list(_wg_cases(WG3, WB3)))
def test_conv3_weight_gradient_lattice(dev, shape, expect, pure16):
    _wgrad(dev, GEOM["conv3"], *shape, "lattice", expect, xdt=BF if pure16 else F32, dydt=BF if pure16 else F32)


@pytest.mark.parametrize("shape,expect,pure16", list(_wg_cases(WG2, WB2)))
def test_conv2_weight_gradient_lattice(dev, shape, expect, pure16):
    _wgrad(dev, GEOM["conv2"], *shape, "lattice", expect, xdt=BF if pure16 else F32, dydt=BF if pure16 else F32)


WG1 = [
    ((3, 44, 44), BF, "conv1_wgrad u8=0 R=10 grid=3"),                     # OW = 10, padded to 16
    ((2, 40, 40), BF, "conv1_wgrad u8=0 R=9 grid=2"),                      # OW = 9: the smallest map the phase-plane kernel takes (7 padding columns)
    ((5, 84, 84), BF, "conv1_wgrad u8=0 R=10 grid=5"),
    ((3, 86, 84), BF, "conv1_wgrad u8=0 R=10 grid=3"),                     # two input rows the stride never reaches
    ((3, 200, 200), BF, "conv1_wgrad u8=0 R=4 grid=3"),
    ((3, 44, 44), F32, "wband<3,1,8,8,4> pure16=0 R=10 F=1 units=3 grid=3"),
    ((5, 84, 84), F32, "wband<3,1,8,8,4> pure16=0 R=20 F=1 units=5 grid=5"),
    ((4, 36, 36), BF, "wgrad_gather f32=0 P=1"),                           # OW = 8: one 8-pixel block per row, left to the generic kernel
    ((2, 40, 40), F32, "wgrad_gather f32=0 P=1"),                          # 81 pixels per frame: under the 96-pixel cut
]


@pytest.mark.parametrize("shape,dydt,expect", WG1, ids=[f"{s}-dy-{str(t).split('.')[-1]}" for s, t, _ in WG1])
def test_conv1_weight_gradient_lattice(dev, shape, dydt, expect):
    _wgrad(dev, GEOM["conv1"], *shape, "lattice", expect, xdt=F32, dydt=dydt)


WG_RANDOM = [
    ("conv3", (2, 9, 9), WB3 + "pure16=1 R=7 F=2 units=1 grid=1", BF, BF),
    ("conv3", (2, 9, 9), WB3 + "pure16=0 R=7 F=2 units=1 grid=1", F32, F32),
    ("conv3", (1, 9, 9), "wgrad_gather f32=0 P=1", BF, BF),
    ("conv2", (2, 20, 20), WB2 + "pure16=1 R=9 F=2 units=1 grid=1", BF, BF),
    ("conv2", (2, 20, 20), WB2 + "pure16=0 R=9 F=2 units=1 grid=1", F32, F32),
    ("conv1", (3, 44, 44), "conv1_wgrad u8=0 R=10 grid=3", F32, BF),
    ("conv1", (3, 44, 44), "wband<3,1,8,8,4> pure16=0 R=10 F=1 units=3 grid=3", F32, F32),
]


@pytest.mark.parametrize("layer,shape,expect,xdt,dydt", WG_RANDOM, ids=[f"{l}-{s}-{_name(e)}" for l, s, e, _, _ in WG_RANDOM])
def test_weight_gradient_random(dev, layer, shape, expect, xdt, dydt):
    _wgrad(dev, GEOM[layer], *shape, "random", expect, xdt=xdt, dydt=dydt)


# ------------------------------------------------------------------------------------------------
# fp32 compute: the gather kernels' float instances
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer,shape", [("conv2", (2, 17, 21)), ("conv3", (2, 11, 13))])
def test_fp32_compute_lattice(dev, layer, shape):
    from hulc2_amd import kernels as kn

    s2 = GEOM[layer][3] ** 2
    _fwd(dev, GEOM[layer], *shape, "lattice", "gather<f32>", xdt=F32, ydt=F32, wdt=F32, compute=kn.F32)
    _dgrad(dev, GEOM[layer], *shape, "lattice", f"gather<f32> launches={s2}", dt=F32, wdt=F32, compute=kn.F32)
    _wgrad(dev, GEOM[layer], *shape, "lattice", "wgrad_gather f32=1 P=1", xdt=F32, dydt=F32, compute=kn.F32)


# ------------------------------------------------------------------------------------------------
# views that are not 16-byte aligned: the direct-to-LDS and conv1 band instances check `% 16` on the host and hand over; the kernels that take
# the call (register-staged bands, gather) use plain global loads, which need element alignment only
# ------------------------------------------------------------------------------------------------
def test_misaligned_inputs_hand_over_and_stay_exact(dev):
    _fwd(dev, GEOM["conv3"], 3, 23, 23, "lattice", BX3 + "multi=0 R=21 F=1 units=3 grid=3", lead=4)
    _fwd(dev, GEOM["conv1"], 3, 44, 44, "lattice", "gather<bf16>", xdt=F32, lead=2)
    _fwd(dev, R18, 1, 56, 56, "lattice", BX3 + "multi=0 R=8 F=1 units=7 grid=7", pad=1, add=True, lead=4)
    _dgrad(dev, GEOM["conv3"], 3, 23, 23, "lattice", BXD3 + "bits=2 multi=0 R=23 F=1 units=3 grid=3", mask="planes", lead=4)
    _dgrad(dev, GEOM["conv2"], 3, 49, 49, "lattice", BXD2 + "xf32=0 bits=2 multi=0 R=25 F=1 units=3 grid=3", mask="planes", lead=4)
    _wgrad(dev, GEOM["conv3"], 3, 23, 23, "lattice", WB3 + "pure16=1 R=11 F=1 units=6 grid=6", lead=4)


# ------------------------------------------------------------------------------------------------
# refusals: the launcher's message, outputs untouched, no path reported
# ------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from hulc2_amd import kernels as kn

    def t(dt, *shape):
        return _in(dev, torch.zeros(*shape, dtype=torch.float64), dt)

    def no_path():
        assert kn.conv_last_path() == ("", {}), f"a refused call reported the path {kn.conv_last_path()}"

    def fwd_refused(msg, N, H, W, Cin, Cout, Kk, s, nchw, xdt=BF, ydt=BF, wdt=BF, **kw):
        kw.setdefault("compute", kn.BF16)
        OH, OW = kn.conv_out_hw(H, W, Kk, Kk, s)
        x = t(xdt, N, Cin, H, W) if nchw else t(xdt, N, H, W, Cin)
        y = out_flat(dev, N * OH * OW * Cout, ydt)
        outs = [y]
        for name in ("relu_bits", "y_bf16"):
            if kw.get(name) is True:
                o = out_flat(dev, N * OH * OW * Cout // (32 if name == "relu_bits" else 1), torch.int32 if name == "relu_bits" else BF)
                kw[name] = o.t.reshape(-1) if name == "relu_bits" else o.t.reshape(N, OH, OW, Cout)
                outs.append(o)
        if kw.get("w_lo") is True:
            kw["w_lo"] = t(BF, Cout, Cin * Kk * Kk)
        refused(lambda: kn.conv2d_fwd(x, t(wdt, Cout, Cin * Kk * Kk), t(F32, Cout), y.t.reshape(N, OH, OW, Cout), N, H, W, Cin, Cout, Kk, Kk, s, nchw, **kw),
                msg, *outs)
        no_path()

    fwd_refused("conv: Cout must be 32 or 64", 2, 20, 20, 32, 48, 4, 2, False)
    fwd_refused("conv: inner run (KW for NCHW input, Cin for NHWC) must be a power of two >= 8", 2, 20, 20, 24, 64, 4, 2, False)
    fwd_refused("conv: too many taps", 1, 20, 20, 32, 64, 9, 1, False)
    fwd_refused("conv: f32 compute requires f32 operands", 2, 20, 20, 32, 64, 4, 2, False, compute=kn.F32)
    fwd_refused("hulc_conv2d_fwd: relu_bits needs relu and Cout % 32 == 0", 2, 20, 20, 32, 64, 4, 2, False, relu=False, relu_bits=True)
    fwd_refused("hulc_conv2d_fwd: an fp16 output is the twin of a bf16 map (y_bf16)", 3, 23, 23, 64, 64, 3, 1, False, ydt=F16)
    fwd_refused("hulc_conv2d_fwd: the fp16 twin is stored by the direct-to-LDS band kernel only", 3, 9, 9, 64, 64, 3, 1, False, ydt=F16, y_bf16=True)
    fwd_refused("hulc_conv2d_fwd: split operands (w_lo) are taken by the conv1 band kernel only", 2, 20, 20, 32, 64, 4, 2, False, w_lo=True)
    # (the Python wrapper refuses these two itself: the descriptor by hand)
    N, H, W = 3, 9, 9
    x, w, b = t(BF, N, H, W, 64), t(BF, 64, 576), t(F32, 64)
    y, y16 = out_flat(dev, N * 7 * 7 * 64, BF), out_flat(dev, N * 7 * 7 * 64, BF)
    d = kn._conv_desc(N, H, W, 64, 64, 3, 3, 1, False, kn.BF16, kn.BF16, kn.BF16, True, kn.BF16)
    d.y_bf16 = y16.t.data_ptr()
    refused(lambda: kn._call("hulc_conv2d_fwd", ctypes.byref(d), x, w, b, y.t), "hulc_conv2d_fwd: y_bf16 goes with an fp32 / fp16 output", y, y16)
    no_path()
    d = kn._conv_desc(N, H, W, 64, 64, 3, 3, 1, False, kn.BF16, kn.BF16, kn.BF16, True, kn.BF16)
    d.x2, d.n_split = x.data_ptr(), N - 1                # (x itself holds all N frames: nothing could be read past it)
    refused(lambda: kn._call("hulc_conv2d_fwd", ctypes.byref(d), x, w, b, y.t), "hulc_conv2d_fwd: a second frame tensor (x2) is taken by the conv1 band kernel only", y)
    no_path()
    dw, db = out_flat(dev, 64 * 576, F32), out_flat(dev, 64, F32)
    xf = t(F32, N, H, W, 64)
    refused(lambda: kn.conv2d_bwd_weight(xf[:N - 1], t(BF, N, 7, 7, 64), dw.t.reshape(64, 576), db.t.reshape(64), N, H, W, 64, 64, 3, 3, 1, False,
                                         compute=kn.BF16, x2=xf[N - 1:]),
            "conv weight gradient: x2 / frame slots are for conv1 only", dw, db)
    no_path()
    # data gradient
    for msg, Cin, nchw in (("conv bwd_data: Cin must be 32 or 64", 16, False), ("hulc_conv2d_bwd_data: only NHWC activations have a data gradient on this path", 32, True)):
        dx = out_flat(dev, 2 * 20 * 20 * Cin, BF)
        d = kn._conv_desc(2, 20, 20, Cin, 64, 4, 4, 2, nchw, kn.BF16, kn.BF16, kn.BF16, False, kn.BF16)
        refused(lambda: kn._call("hulc_conv2d_bwd_data", ctypes.byref(d), t(BF, 2, 9, 9, 64), t(BF, Cin, 4, 4, 64), dx.t, None), msg, dx)
        no_path()
    # conv1's frame sources (x2 / n_split / x_slot / x2_slot), which both conv1 band launchers judge, each with its own message — and its own
    # order where two apply: the forward names the slots first, the weight gradient x2.  The smallest frames the band kernels take; x holds all
    # N frames and the slot x's address, so no field points anywhere a launch could not read.  (the Python wrappers never build these.)
    N, H, W = 2, 24, 24
    x, xu8 = t(F32, N, 3, H, W), torch.zeros(N, H, W, 3, dtype=torch.uint8, device=dev)
    slot = torch.tensor([x.data_ptr()], dtype=torch.int64, device=dev)
    SLOTS = "frame slots are for fp32 frames (x_slot with every launch, x2_slot next to x2), 8-byte aligned"

    def conv1_desc(ydt, u8=False, **fields):
        d = kn._conv_desc(N, H, W, 3, 32, 8, 8, 4, True, kn.F32, ydt, kn.BF16, True, kn.BF16)
        d.x_u8_nhwc = int(u8)
        for k, v in fields.items():
            setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        return d

    w, b, y = t(BF, 32, 192), t(F32, 32), out_flat(dev, N * 5 * 5 * 32, BF)
    for msg, xin, d in (
            ("conv1 band: x2 needs 0 <= n_split <= N", x, conv1_desc(kn.BF16, x2=x, n_split=N + 1)),
            ("conv1 band: x2 needs 0 <= n_split <= N", x, conv1_desc(kn.BF16, x2=x, n_split=-1)),
            ("conv1 band: " + SLOTS, xu8, conv1_desc(kn.BF16, u8=True, x_slot=slot)),
            ("conv1 band: " + SLOTS, x, conv1_desc(kn.BF16, x_slot=slot, x2_slot=slot)),
            ("conv1 band: " + SLOTS, x, conv1_desc(kn.BF16, x2=x, n_split=N + 1, x2_slot=slot))):
        refused(lambda: kn._call("hulc_conv2d_fwd", ctypes.byref(d), xin, w, b, y.t), msg, y)
        no_path()
    dw, db = out_flat(dev, 32 * 192, F32), out_flat(dev, 32, F32)
    ws = torch.empty(kn._L.load().hulc_conv2d_bwd_weight_workspace(ctypes.byref(conv1_desc(kn.BF16))) // 4, dtype=F32, device=dev)
    for msg, xin, dydt, d in (
            ("conv1 weight gradient: x2 needs a bf16 gradient map", x, F32, conv1_desc(kn.F32, x2=x, n_split=1)),
            ("conv1 weight gradient: x2 needs a bf16 gradient map", x, BF, conv1_desc(kn.BF16, x2=x, n_split=N + 1)),
            ("conv1 weight gradient: x2 needs a bf16 gradient map", x, BF, conv1_desc(kn.BF16, x2=x, n_split=N + 1, x2_slot=slot)),
            ("conv1 weight gradient: frame slots need the phase-plane kernel (bf16 gradient map)", x, F32, conv1_desc(kn.F32, x_slot=slot)),
            ("conv1 weight gradient: " + SLOTS, xu8, BF, conv1_desc(kn.BF16, u8=True, x_slot=slot)),
            ("conv1 weight gradient: " + SLOTS, x, BF, conv1_desc(kn.BF16, x_slot=slot, x2_slot=slot))):
        refused(lambda: kn._call("hulc_conv2d_bwd_weight", ctypes.byref(d), xin, t(dydt, N, 5, 5, 32), dw.t, db.t, ws), msg, dw, db)
        no_path()
