"""Kernel-level tests of the padded-grid family (csrc/gridconv.hip, affordance.hip, wgrad_taps.hip) through the C ABI on tensors the test
owns, every kernel instance against float64.  The pattern of a case and the tolerance rule are in tests/kcheck.py, the grid fixture
(`GridBuf`) and the replays of the launchers' host arithmetic in tests/gridref.py; what is particular to this file:

GRIDS.  Every grid tensor is a `GridBuf`: sentinel | exactly W + 3 zero rows | the R rows | exactly (Rpad - R) + W + 3 zero rows | sentinel,
padding columns (ld > C) sentinel, an OUTPUT's R rows sentinel.  A read past the promised guard that reaches a result is a NaN, a write
outside the R x C block fails assert_guards, a border row the kernel promises to zero but skips stays NaN.

LATTICE cases.  Activations and gradients integers in [-3, 3], weights integers in [-3, 3] / 8, biases and accumulate bases multiples of 1/8 in
[-2, 2], the fusion vector g multiples of 1/4 in [-2, 2]: every fp32 partial sum is a multiple of 2^-3 (2^-6 for the y^2 statistics) and exact
whatever the order while it stays below 2^24 units — each case asserts that from its float64 reference (statistics: per 128-row tile, and over
all tiles wherever the test or a kernel sums tiles).  A bf16 output equals the float64 value rounded once, fp32 outputs equal it bit for bit.

RANDOM cases.  Seeded float64 operands rounded to the storage type, compare() / compare_rows() with the same formula in CPU float32 as the
yardstick.

PATH.  Every gridconv case names the instance it means to hit and asserts the launcher's report (kernels.conv_last_path()) against the replay of
gridconv_launch's dispatch; multi-trip, multi-group and multi-slab cases assert from the replayed arithmetic that they reach that path."""
import pytest
import torch
import torch.nn.functional as F

from tests import gridref as G
from tests import kcheck as K
from tests.gridref import GridBuf
from tests.kcheck import Guarded, compare, compare_rows, out_flat, refused, rnd, same_bits

pytestmark = pytest.mark.gpu

# Margins of margin * max(e_ref, 2^-23), e_ref = the same formula in CPU float32 against float64 (tests/kcheck.py).
#   SUM 4: products of bf16 operands are exact in fp32, only the order of the fp32 sums (and single roundings of pointwise formulas) differ.
# A kernel that cannot meet 4 is a finding and gets a row here with the measured float32-CPU and GPU errors and the cause; its margin is then at
# most the project's other class (16).
#   kernel                        what     cpu-f32     gpu        cause
#   depth_nll_fwd (B = 4096)      loss     5.1e-09     1.08e-06   ratio 9.09: one workgroup, each of its four waves adds its 1,024 per-row terms one
#                                                                 after the other in fp32 (error grows with the count, and a few terms near
#                                                                 r^2 / 1e-6 carry the sum) where torch's CPU mean adds pairwise; no term is lost.
#                                                                 B <= 70: ratio at most 1.40.  Class SEQ for this scalar alone; mu, sigma, log_sigma stay SUM.
# Largest ratios measured on an MI355X (K.report): gridconv<2,2,4> 2.48 (fused 2.17), <1,1,1> 1.67, <1,2,1> 1.53, <1,1,2> 1.50, <1,2,2> 1.42,
# <2,2,1> 1.39, <2,2,2> 1.08, thin<32,1> 1.15, thin<32,2> 0.95, thin<64,1> 1.42; grid_bn_finalize 0.84 (G = 1) / 0.74 (G > 1);
# grid_bn_relu_bwd 1.20 / 1.29; pixel_ce_fwd 0.50, pixel_ce_bwd_rows 0.54, pixel_ce_bwd 0.00 (the bf16 output's half ulp covers __expf: no row
# needed); depth_nll_bwd 3.03; depth_nll_fwd 9.09 (the loss above; 2.62 without it); every lattice case 0 by construction.
MARGIN = {"SUM": 4.0, "SEQ": 16.0}

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32


@pytest.fixture(scope="module", autouse=True)
def _module():
    from hulc2_amd import kernels as kn
    kn.set_compute("bf16")
    yield
    K.report("tests/test_grid_kernels_gpu.py")


def _kn():
    from hulc2_amd import kernels as kn
    return kn


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


def _in(dev, t64, dtype=F32, lead=0):
    """an input tensor inside a NaN-sentinel allocation"""
    return out_flat(dev, t64.numel(), dtype, init=t64, lead=lead).t.reshape(t64.shape)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _row(name):
    K.RATIOS.setdefault(name, 0.0)


def _units(top, unit, what):
    assert top / unit < 2 ** 24, f"{what}: the largest sum is {top / unit:.0f} units of {unit:g}, not below 2^24: the lattice is no longer exact in fp32"


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} against {want.dtype} {tuple(want.shape)}"
    g, w = got.cpu(), want.cpu()
    assert torch.equal(g, w), (f"{what}: {(g != w).sum().item()} of {g.numel()} elements differ from the float64 reference "
                               f"(max abs difference {(g.double() - w.double()).abs().max().item():.3e}, non-finite {(~torch.isfinite(g.float())).sum().item()})")


# ------------------------------------------------------------------------------------------------
# 1. hulc_gridconv3x3 / hulc_gridconv3x3_fused
# ------------------------------------------------------------------------------------------------
def _conv_ref(a_nchw, w4, flip, dt):
    """not flip: conv2d(a, w4 (Cout, Cin, 3, 3)); flip: the data gradient of conv2d(., w4 (Cin_k, Cout_k, 3, 3)) for the output gradient a"""
    a_nchw, w4 = a_nchw.to(dt), w4.to(dt)
    if not flip:
        return F.conv2d(a_nchw, w4, padding=1)
    xz = torch.zeros(a_nchw.shape[0], w4.shape[1], *a_nchw.shape[2:], dtype=dt, requires_grad=True)
    F.conv2d(xz, w4, padding=1).backward(a_nchw)
    return xz.grad


def _conv_case(dev, N, H, W, Cin, Cout, inst, mode="lattice", flip=False, stats=False, out0=None, xpad=0, ypad=0, fused=None, addpad=0, hi=3,
               total=True):
    """one hulc_gridconv3x3 (fused: hulc_gridconv3x3_fused with (bias, add, relu)) call, twice.  inst: the kernel instance the case means to hit;
    out0: None / "both" (next to y) / "only" (y == NULL); xpad / ypad / addpad: extra pitch; total: the statistics' exactness is also asserted
    over all tiles (off only where nothing sums the tiles)"""
    kn = _kn()
    what = f"gridconv {(N, H, W, Cin, Cout)} {inst} {mode} flip={flip} stats={stats} out0={out0} fused={fused} pads={(xpad, ypad, addpad)}"
    g = _gen("gridconv", N, H, W, Cin, Cout, mode, flip, fused)
    R, inner = G.grid_R(N, H, W), G.interior_mask(N, H, W)
    wshape = (Cin, Cout, 3, 3) if flip else (Cout, Cin, 3, 3)
    use_bias, use_add, relu = fused if fused else (False, False, False)
    if mode == "lattice":
        a64, w64 = _ints(g, N, Cin, H, W, lo=-hi, hi=hi), _ints(g, *wshape) / 8          # no symmetry between taps, none between ci and co
        cb64 = _ints(g, Cout, lo=-16, hi=16) / 8
        add64 = _ints(g, N, Cout, H, W)
        b0 = _ints(g, 1, lo=-16, hi=16) / 8
    else:
        a64, w64 = rnd(_uni(g, N, Cin, H, W), BF), rnd(_uni(g, *wshape) / (9 * Cin) ** 0.5, BF)
        cb64, add64, b0 = rnd(_uni(g, Cout) * 0.1, F32), rnd(_uni(g, N, Cout, H, W), BF), rnd(_uni(g, 1), F32)
    wt64 = G.dgrad_weights(w64) if flip else G.fwd_weights(w64)
    assert tuple(wt64.shape) == (Cout, 9 * Cin)

    def ref(dt):
        z = _conv_ref(a64, w64, flip, dt)
        if use_bias:
            z = z + cb64.to(dt)[None, :, None, None]
        if use_add:
            z = z + add64.to(dt)
        if relu:
            z = torch.relu(z)
        return G.to_rows(_nhwc(z))

    v64 = ref(torch.float64)
    x = GridBuf(dev, N, H, W, Cin, ld=Cin + xpad, rows64=G.to_rows(_nhwc(a64)))
    wt = _in(dev, wt64, BF)
    addb = GridBuf(dev, N, H, W, Cout, ld=Cout + addpad, rows64=G.to_rows(_nhwc(add64))) if use_add else None
    cb = _in(dev, cb64) if use_bias else None
    bias0 = _in(dev, b0)
    nb = (R + G.TILE - 1) // G.TILE
    expect = G.gridconv_path(Cin, Cout, R, _cus(), ldy=(Cout + ypad) if out0 != "only" else 0)
    assert expect.startswith(inst + " "), f"{what}: the replayed dispatch gives {expect}"
    name = inst + (" fused" if fused else "")

    def call():
        y = GridBuf(dev, N, H, W, Cout, ld=Cout + ypad) if out0 != "only" else None
        st = Guarded(dev, nb * 2, Cout) if stats else None
        o0 = out_flat(dev, R) if out0 else None
        if fused:
            kn._call("hulc_gridconv3x3_fused", x.t, x.ld, wt, y.t, y.ld, N, H, W, Cin, Cout, cb, addb.t if use_add else None, addb.ld if use_add else 0, int(relu))
        else:
            kn._call("hulc_gridconv3x3", x.t, x.ld, wt, y.t if y else None, y.ld if y else 0, N, H, W, Cin, Cout, int(flip), st.t if stats else None,
                     o0.t if out0 else None, bias0 if out0 else None)
        got = kn.conv_last_path()
        assert got == kn_plan(expect), f"{what}: served by {got}, the case means to hit {expect}"
        torch.cuda.synchronize()
        for o, nm in ((y, "y"), (st, "stats"), (o0, "out0")):
            if o is not None:
                o.assert_guards(f"{what} {nm}")
        return (y.value() if y else None, st.value().reshape(nb, 2, Cout) if stats else None, o0.value().reshape(-1) if out0 else None)

    y, st, o0 = call()
    _row(name)
    if relu:
        frac = (v64[inner] > 0).double().mean().item()
        assert 0.2 < frac < 0.8, f"{what}: {frac:.2f} of the outputs are positive, the ReLU means nothing"
    want0 = torch.where(inner, v64[:, 0] + b0[0], torch.zeros(()).double())
    if mode == "lattice":
        _units(9 * Cin * hi * 3 / 8 + 2 + 3, 2.0 ** -3, what + " (sum of magnitudes)")
        _units(v64.abs().max().item() + 2, 2.0 ** -3, what)
        if y is not None:
            _equal(y, v64.float().to(BF).to(dev), what + " y")
        if out0:
            _equal(o0, want0.float(), what + " out0")
        if stats:
            sp = G.stats_partials(v64, N, H, W)
            _units(sp[:, 0].abs().max().item(), 2.0 ** -3, what + " tile sums of y")
            _units(sp[:, 1].max().item(), 2.0 ** -6, what + " tile sums of y^2")
            if total:
                _units(sp[:, 1].sum(0).max().item(), 2.0 ** -6, what + " sum of y^2 over all tiles")
            _equal(st, sp.float(), what + " stats")
    else:
        v32 = ref(torch.float32)
        if y is not None:
            assert not G.borders(y, N, H, W).float().any(), f"{what}: border rows of y are not zero"
            compare(name, "y", y[inner.to(dev)], v64[inner], v32[inner], MARGIN["SUM"], out_dtype=BF)
        if out0:
            assert not o0[~inner.to(dev)].any(), f"{what}: border rows of out0 are not zero"
            compare(name, "out0", o0, want0, torch.where(inner, v32[:, 0] + b0[0].float(), torch.zeros(())), MARGIN["SUM"])
        if stats:
            sp, sp32 = G.stats_partials(v64, N, H, W), G.stats_partials(v32, N, H, W)
            compare(name, "stats y", st[:, 0], sp[:, 0], sp32[:, 0], MARGIN["SUM"])
            compare(name, "stats y^2", st[:, 1], sp[:, 1], sp32[:, 1], MARGIN["SUM"])
    y2, st2, o02 = call()
    for a, b, nm in ((y, y2, "y"), (st, st2, "stats"), (o0, o02, "out0")):
        if a is not None:
            same_bits(a, b, f"{what} {nm}")


def kn_plan(text):
    words = text.split()
    return words[0], {k: int(v) for k, v in (w.split("=") for w in words[1:])}


T11, T12, T61 = "gridconv_thin<32,1>", "gridconv_thin<32,2>", "gridconv_thin<64,1>"
# id: (N, H, W, Cin, Cout, instance, options).  R % 128 != 0 everywhere; R < 128 at least once per kernel template (56 / 112 rows)
CONV_CASES = {
    "thin32x32": (2, 11, 7, 32, 32, T11, dict(stats=True, out0="both")),                       # R = 234
    "thin32x32-small-out0only": (1, 6, 5, 32, 32, T11, dict(out0="only")),                     # R = 56, y == NULL
    "thin32x64": (2, 9, 9, 32, 64, T12, dict(stats=True, xpad=32, ypad=8)),                    # R = 242, the cin= use, ldy > Cout
    "thin64x32": (2, 6, 5, 64, 32, T61, dict(stats=True, ypad=16)),                            # R = 112
    "g224": (1, 6, 5, 256, 128, "gridconv<2,2,4>", dict(stats=True)),                          # R = 56
    "g224-4tiles": (2, 14, 13, 256, 128, "gridconv<2,2,4>", dict(stats=True, ypad=8)),         # R = 480
    "g222": (2, 7, 7, 128, 128, "gridconv<2,2,2>", dict(ypad=8, out0="both")),                 # R = 162
    "g221": (3, 5, 5, 96, 128, "gridconv<2,2,1>", dict(xpad=32, stats=True)),                  # R = 147
    "g122": (2, 7, 6, 128, 64, "gridconv<1,2,2>", dict(stats=True, ypad=8)),                   # R = 144
    "g122-192": (1, 6, 5, 192, 192, "gridconv<1,2,2>", dict()),                                # three column blocks, R = 56
    "g121": (2, 6, 5, 64, 64, "gridconv<1,2,1>", dict(stats=True, xpad=64)),                   # R = 112
    "g112": (2, 7, 6, 128, 32, "gridconv<1,1,2>", dict(stats=True, out0="both")),              # R = 144
    "g112-96": (1, 6, 5, 128, 96, "gridconv<1,1,2>", dict(ypad=32)),                           # R = 56
    "g111-96x32-out0only": (2, 9, 9, 96, 32, "gridconv<1,1,1>", dict(out0="only", stats=True)),     # R = 242
    "g111-96x96": (1, 6, 5, 96, 96, "gridconv<1,1,1>", dict(xpad=32)),                         # R = 56
    # thin shapes the launcher must send to the generic kernel: 16-byte stores of the output tile need ldy % 8 == 0
    "forced32x32": (2, 11, 7, 32, 32, "gridconv<1,1,1>", dict(ypad=4, stats=True)),
    "forced32x64": (2, 9, 9, 32, 64, "gridconv<1,2,1>", dict(ypad=4)),
    "forced64x32": (2, 6, 5, 64, 32, "gridconv<1,1,1>", dict(ypad=12, out0="both")),
}


@pytest.mark.parametrize("flip", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("case", list(CONV_CASES))
def test_gridconv_lattice(dev, case, flip):
    """every instance: the forward and the flip_taps data gradient (weights as dgrad_weights) against conv2d and its autograd, bit for bit"""
    N, H, W, Cin, Cout, inst, opt = CONV_CASES[case]
    _conv_case(dev, N, H, W, Cin, Cout, inst, flip=flip, **opt)


@pytest.mark.parametrize("case", ["thin32x32", "thin32x64", "thin64x32", "g224", "g222", "g221", "g122", "g121", "g112", "g111-96x32-out0only", "forced32x32"])
def test_gridconv_random(dev, case):
    N, H, W, Cin, Cout, inst, opt = CONV_CASES[case]
    _conv_case(dev, N, H, W, Cin, Cout, inst, mode="random", **opt)


FUSED = {"bias+add+relu": (True, True, True), "bias+relu": (True, False, True), "bias+add": (True, True, False)}


@pytest.mark.parametrize("mode,fused", [("lattice", k) for k in FUSED] + [("random", "bias+add+relu")])
@pytest.mark.parametrize("shape,inst,opt", [((2, 12, 10, 32, 32), T11, dict(addpad=8)), ((2, 9, 9, 32, 64), T12, dict(addpad=32, ypad=8)),
                                            ((3, 6, 5, 64, 32), T61, dict(addpad=8)), ((2, 7, 6, 128, 64), "gridconv<1,2,2>", dict(addpad=8, ypad=8)),
                                            ((1, 14, 13, 256, 256), "gridconv<2,2,4>", dict(addpad=16)), ((2, 7, 7, 96, 96), "gridconv<1,1,1>", dict(addpad=32))],
                         ids=["thin32x32", "thin32x64", "thin64x32", "g122", "g224", "g111"])
def test_gridconv_fused_epilogue(dev, shape, inst, opt, fused, mode):
    """the BasicBlock epilogue (bias, residual rows ldadd > Cout apart, ReLU) in the three combinations the frozen trunk uses, bit for bit; the
    full epilogue once more on random operands"""
    _conv_case(dev, *shape, inst, mode=mode, fused=FUSED[fused], **opt)


def _two_trip_N(Cin, Cout, HW):
    """the smallest N at which a workgroup of the thin instance takes a second trip of its persistent loop, from the launcher's arithmetic:
    csrc/gridconv.hip GT_LAUNCH `wgs = ((OCC * ncu + 7) / 8) * 8` and gridconv_thin_kernel `per = (ntiles + 7) / 8`, `nslots = gridDim.x >> 3`,
    `next = tile + nslots; more = next < tend`"""
    plan = kn_plan(G.gridconv_path(Cin, Cout, 128, _cus()))[1]
    for N in range(1, 64):
        per, nslots = G.thin_trips((G.grid_R(N, HW, HW) + 127) // 128, plan["wgs"])
        if per > nslots:
            return N, per, nslots
    raise AssertionError("no N below 64 gives a second trip")


@pytest.mark.parametrize("Cin,Cout,HW,inst", [(32, 32, 156, T11), (32, 64, 130, T12), (64, 32, 130, T61)], ids=["32x32", "32x64", "64x32"])
def test_gridconv_thin_second_trip_lattice(dev, Cin, Cout, HW, inst):
    """a second trip of the persistent loop reuses the prefetched windows and rewrites rowok, outs and sred behind the closing barrier: lattice
    operands, so a stale window or a torn tile is a wrong integer.  (On 256 CUs: N = 4; 545 tiles at 130 x 130 are 69 per XCD against 64 slots,
    781 tiles at 156 x 156 are 98 against the 96 slots of the 32 -> 32 instance.)  The statistics are asserted exact per tile only: nothing in
    this case sums the tiles."""
    N, per, nslots = _two_trip_N(Cin, Cout, HW)
    assert per > nslots, f"{per} tiles per XCD on {nslots} slots: no workgroup takes a second trip"
    assert N <= 8, f"{_cus()} CUs need N = {N} for a second trip: not a quick case any more"
    _conv_case(dev, N, HW, HW, Cin, Cout, inst, stats=True, total=False)


# ------------------------------------------------------------------------------------------------
# 2. nine-tap weight gradient (conv_taps_wp items of hulc_wgrad_group, csrc/wgrad_taps.hip)
# ------------------------------------------------------------------------------------------------
def _taps_case(dev, N, H, W, Cin, Cout, hi=3, want_split=None):
    """dW (Cout, Cin, 3, 3) = sum over grid rows of dZ^T X[. + off_u]: store, accumulate on a lattice base, store_rows = 1 (Cout == 32), each twice"""
    kn = _kn()
    what = f"nine-tap wgrad {(N, H, W, Cin, Cout)}"
    g = _gen("taps", N, H, W, Cin, Cout)
    x64, dz64 = _ints(g, N, Cin, H, W, lo=-hi, hi=hi), _ints(g, N, Cout, H, W)
    base64 = _ints(g, Cout, Cin * 9, lo=-16, hi=16) / 8
    X = GridBuf(dev, N, H, W, Cin, rows64=G.to_rows(_nhwc(x64)), pad32=True)
    DZ = GridBuf(dev, N, H, W, Cout, rows64=G.to_rows(_nhwc(dz64)), pad32=True)
    Kr = X.Rpad
    # csrc/wgrad_taps.hip hulc_wgrad_taps_takes: the shapes the nine-tap kernel takes (others run as nine plain items)
    assert (Cout % 64 == 0 or Cout == 32) and (Cin % 64 == 0 or Cin == 32) and Kr % 32 == 0 and Kr >= 64
    plan = G.plan_taps(Cout, Cin, Kr)                            # csrc/wgrad_taps.hip plan_taps: M = Cout, N = Cin, K = padded rows
    if want_split is not None:
        assert want_split(plan["ksplit"]), f"{what}: plan {plan} does not reach the path this case is about"
    if N * H * W <= 20000:
        wz = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(x64, wz, padding=1).backward(dz64)
        ref = wz.grad.reshape(Cout, Cin * 9)
    else:                                                        # (the same sums as nine products over the grid rows: tests/test_gridref_cpu.py)
        ref = G.taps_wgrad_rows(G.to_rows(_nhwc(dz64)), G.to_rows(_nhwc(x64)), W).reshape(Cout, Cin * 9)
    _units(N * H * W * 3 * hi + 2, 2.0 ** -3, what + " (sum of magnitudes)")
    name = f"wgrad_taps mode={plan['mode']}" + (" split" if plan["ksplit"] > 1 else "") + (" 2-level" if plan["ksplit"] > 16 else "")
    _row(name)

    def call(accumulate, store_rows=0):
        rows = store_rows or Cout
        dw = Guarded(dev, rows, Cin * 9, init=base64[:rows])
        kn.wgrad(DZ.t, X.t, dw.t, Cout, Cin, Kr, DZ.ld, X.ld, Cin * 9, accumulate=accumulate, col_mul=9, store_rows=store_rows, conv_taps_wp=W + 2)
        torch.cuda.synchronize()
        dw.assert_guards(f"{what} dW accumulate={accumulate} store_rows={store_rows}")
        return dw.value()

    for accumulate, rows in ((False, 0), (True, 0)) + (((False, 1),) if Cout == 32 else ()):
        want = (ref + (base64 if accumulate else 0))[:rows or Cout].float().to(dev)
        got = call(accumulate, rows)
        _equal(got, want, f"{what} dW accumulate={accumulate} store_rows={rows}")
        same_bits(got, call(accumulate, rows), f"{what} dW accumulate={accumulate} store_rows={rows}")


@pytest.mark.parametrize("shape", [(1, 7, 7, 64, 64), (1, 7, 7, 32, 32), (1, 7, 7, 64, 32), (1, 7, 7, 32, 64), (1, 7, 7, 128, 64), (1, 30, 17, 192, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_nine_tap_weight_gradient_lattice(dev, shape):
    """every wave arrangement (64 x 64 blocks, M == 32, N == 32, both) at 96 rows (the last k-step half empty) and one multi-tile item"""
    _taps_case(dev, *shape, want_split=lambda k: k == 1)


def test_nine_tap_weight_gradient_split_lattice(dev):
    """64 -> 64 at 2 x 46 x 46: 72 k-steps, two slices through the slabs"""
    _taps_case(dev, 2, 46, 46, 64, 64, want_split=lambda k: 1 < k <= 16)


def test_nine_tap_weight_gradient_second_reduce_level_lattice(dev):
    """64 -> 64 at 1 x 255 x 255: 1,033 k-steps, ksplit 17 — slice group 0 of wgrad_taps_reduce_kernel (`for (s = sg; s < ksplit; s += 16)`) sums
    two slabs.  Activations in [-1, 1] keep the 65,025-pixel sums below 2^24 units of 1/8."""
    _taps_case(dev, 1, 255, 255, 64, 64, hi=1, want_split=lambda k: k > 16)


# ------------------------------------------------------------------------------------------------
# 3. hulc_grid_bn_finalize
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,C,shared,G_want", [(5, 64, True, 1), (7, 32, True, 1), (23, 96, False, 1), (128, 64, True, 2), (128, 96, True, 2),
                                                (2048, 32, True, 32), (2048, 96, True, 32), (2048, 64, False, 1)])
def test_grid_bn_finalize(dev, nb, C, shared, G_want):
    """partials from the test (integers: both sums exact in any order); shared = mid and counters given.  G from the launcher's arithmetic"""
    kn = _kn()
    what = f"grid_bn_finalize nb={nb} C={C} shared={shared}"
    Gr = G.bn_groups(nb, shared)
    assert Gr == G_want, f"{what}: the launcher's arithmetic gives {Gr} row groups"
    name = "grid_bn_finalize " + ("G=1" if Gr == 1 else "G>1")
    g = _gen("bnfin", nb, C)
    part64 = torch.stack([_ints(g, nb, C, lo=-64, hi=64), _ints(g, nb, C, lo=2000, hi=4000)], 1)          # (nb, 2, C)
    count = 1 << 17                                              # a power of two: mean = S1 / count is exact in fp32
    S = part64.sum(0)
    _units(S[1].max().item(), 1.0, what)
    gamma64, beta64 = rnd(_uni(g, C) + 1.5, F32), rnd(_uni(g, C), F32)
    rm64, rv64 = rnd(_uni(g, C), F32), rnd(_uni(g, C) + 2, F32)
    eps, mom = 1e-5, 0.1

    def ref(dt):
        s1, s2, cnt = S[0].to(dt), S[1].to(dt), torch.tensor(float(count), dtype=dt)
        e, m = torch.tensor(eps, dtype=torch.float32).to(dt), torch.tensor(mom, dtype=torch.float32).to(dt)
        mean = s1 / cnt
        var = (s2 / cnt - mean * mean).clamp_min(0)
        rstd = 1 / torch.sqrt(var + e)
        scale = gamma64.to(dt) * rstd
        return dict(mean=mean, rstd=rstd, scale=scale, shift=beta64.to(dt) - mean * scale, run_mean=(1 - m) * rm64.to(dt) + m * mean,
                    run_var=(1 - m) * rv64.to(dt) + m * var * (cnt / (cnt - 1)))

    r64, r32 = ref(torch.float64), ref(torch.float32)
    part, gamma, beta = _in(dev, part64), _in(dev, gamma64), _in(dev, beta64)
    ctr = Guarded(dev, 1, (C + 63) // 64, I32, init=torch.zeros((C + 63) // 64))
    mid = Guarded(dev, 64, C)

    def call():
        bn, rm, rv = Guarded(dev, 4, C), out_flat(dev, C, init=rm64), out_flat(dev, C, init=rv64)
        kn._call("hulc_grid_bn_finalize", part, nb, C, count, gamma, beta, eps, mom, bn.t, rm.t, rv.t, mid.t if shared else None, ctr.t if shared else None)
        torch.cuda.synchronize()
        for o, nm in ((bn, "bn"), (rm, "run_mean"), (rv, "run_var"), (mid, "mid"), (ctr, "counters")):
            o.assert_guards(f"{what} {nm}")
        assert not ctr.value().any(), f"{what}: the counters do not read zero after the call"
        return bn.value(), rm.value().reshape(-1), rv.value().reshape(-1)

    bn, rm, rv = call()
    _equal(bn[0].double() * count, S[0].to(dev), what + " mean * count")
    for i, k in enumerate(("mean", "rstd", "scale", "shift")):
        compare(name, k, bn[i], r64[k], r32[k], MARGIN["SUM"])
    compare(name, "run_mean", rm, r64["run_mean"], r32["run_mean"], MARGIN["SUM"])
    compare(name, "run_var", rv, r64["run_var"], r32["run_var"], MARGIN["SUM"])
    bn2, rm2, rv2 = call()                                       # the same counters again
    for a, b, nm in ((bn, bn2, "bn"), (rm, rm2, "run_mean"), (rv, rv2, "run_var")):
        same_bits(a, b, f"{what} {nm}")


# ------------------------------------------------------------------------------------------------
# 4. hulc_grid_bn_relu_fwd / _bwd
# ------------------------------------------------------------------------------------------------
def _bn_table(g, y_px64, C):
    """(4, C) fp32-representable table (mean, rstd, scale, shift) of BatchNorm over the pixels y_px64 (P, C), and gamma"""
    gamma = rnd(_uni(g, C) * 0.5 + 1.0, F32)
    beta = rnd(_uni(g, C) * 0.3, F32)
    mean = rnd(y_px64.mean(0), F32)
    rstd = rnd(1 / torch.sqrt(y_px64.var(0, unbiased=False) + 1e-5), F32)
    scale = rnd(gamma * rstd, F32)
    shift = rnd(beta - mean * scale, F32)
    return torch.stack([mean, rstd, scale, shift])


@pytest.mark.parametrize("N,H,W,C,pads", [(2, 7, 5, 32, (0, 0)), (3, 5, 4, 96, (32, 8)), (1, 20, 17, 64, (8, 64))], ids=["C32", "C96-pitched", "C64-R418"])
def test_grid_bn_relu_fwd_lattice(dev, N, H, W, C, pads):
    """y integers, scale multiples of 1/4, shift multiples of 1/8: relu(y scale + shift) is exact, the bf16 output one rounding; border rows zero"""
    kn = _kn()
    what = f"grid_bn_relu_fwd {(N, H, W, C)} pads={pads}"
    g = _gen("bnfwd", N, H, W, C)
    y64 = G.to_rows(_ints(g, N, H, W, C, lo=-12, hi=12))
    bn64 = torch.stack([_uni(g, C), _uni(g, C), _ints(g, C, lo=-8, hi=8) / 4, _ints(g, C, lo=-16, hi=16) / 8])          # (mean, rstd: not read)
    inner = G.interior_mask(N, H, W)
    want = torch.where(inner[:, None], torch.relu(y64 * bn64[2] + bn64[3]), torch.zeros(()).double())
    y = GridBuf(dev, N, H, W, C, ld=C + pads[0], rows64=y64)
    bn = _in(dev, rnd(bn64, F32))
    _row("grid_bn_relu_fwd")

    def call():
        out = GridBuf(dev, N, H, W, C, ld=C + pads[1])
        kn._call("hulc_grid_bn_relu_fwd", y.t, y.ld, bn, N, H, W, C, out.t, out.ld)
        torch.cuda.synchronize()
        out.assert_guards(what)
        return out.value()

    out = call()
    _equal(out, want.float().to(BF).to(dev), what)
    same_bits(out, call(), what)


BWD_CASES = {  # N, H, W, C, (dout, out, y, dz) extra pitch, accumulate, counters, G of the sums kernel
    "C32": (2, 7, 5, 32, (0, 0, 0, 0), False, True, 1),
    "C96-pitched-acc": (3, 12, 12, 96, (32, 8, 16, 24), True, True, 1),                       # R = 588: three 256-row blocks, the last ragged
    "C64-nocounters-acc": (2, 9, 9, 64, (0, 8, 0, 8), True, False, 1),
    "C32-two-groups": (2, 126, 126, 32, (0, 0, 0, 0), False, True, 2),                        # R = 32768 = 128 blocks of 256 rows: G = 2
    "C96-two-groups-acc": (1, 180, 180, 96, (0, 0, 0, 0), True, True, 2),                     # R = 33124: 130 blocks, the last ragged
}


@pytest.mark.parametrize("case", list(BWD_CASES))
def test_grid_bn_relu_bwd(dev, case):
    """independent of the forward kernel: `out` is the float64 forward rounded to bf16.  dout integers: dbeta bit for bit; dgamma compare();
    dz compare_rows() per grid row against the CPU float32 formula rounded to bf16; border rows of dz exactly zero"""
    kn = _kn()
    N, H, W, C, pads, acc, counters, G_want = BWD_CASES[case]
    what = f"grid_bn_relu_bwd {case}"
    R, inner = G.grid_R(N, H, W), G.interior_mask(N, H, W)
    nb = (R + 255) // 256                                        # csrc/affordance.hip hulc_grid_bn_relu_bwd: `nb = (R + 255) / 256`
    assert G.bn_groups(nb, counters) == G_want, f"{what}: {nb} partial rows give {G.bn_groups(nb, counters)} row groups"
    name = "grid_bn_relu_bwd " + ("G=1" if G_want == 1 else "G>1")
    g = _gen("bnbwd", case)
    ypx = rnd(_uni(g, N, H, W, C) * 2 + 0.3, BF)
    y64 = G.to_rows(ypx)
    bn64 = _bn_table(g, ypx.reshape(-1, C), C)
    out64 = rnd(torch.where(inner[:, None], torch.relu(y64 * bn64[2] + bn64[3]), torch.zeros(()).double()), BF)
    frac = (out64[inner] > 0).double().mean().item()
    assert 0.2 < frac < 0.8, f"{what}: {frac:.2f} of the outputs are positive, the ReLU mask means nothing"
    dout64 = G.to_rows(_ints(g, N, H, W, C))
    base64 = _ints(g, 2, C, lo=-16, hi=16) / 8
    M = N * H * W

    def ref(dt, round_out):
        d = torch.where(out64 > 0, dout64, torch.zeros(()).double()).to(dt) * inner[:, None].to(dt)
        mean, rstd, scale = bn64[0].to(dt), bn64[1].to(dt), bn64[2].to(dt)
        xh = (y64.to(dt) - mean) * rstd
        s1, s2 = d.sum(0), (d * xh * inner[:, None].to(dt)).sum(0)
        inv = torch.tensor(1.0, dtype=dt) / M
        dz = scale * (d - s1 * inv - xh * s2 * inv) * inner[:, None].to(dt)
        return s1, s2, (dz.to(BF) if round_out else dz)

    s1, s2, dz64 = ref(torch.float64, False)
    _, s2_32, dz32 = ref(torch.float32, True)
    _units(dout64.abs().sum(0).max().item() + 2, 2.0 ** -3, what + " dbeta")
    bufs = [GridBuf(dev, N, H, W, C, ld=C + p, rows64=v) for p, v in zip(pads[:3], (dout64, out64, y64))]
    bn = _in(dev, bn64)
    ctr = Guarded(dev, 1, (C + 63) // 64, I32, init=torch.zeros((C + 63) // 64))
    ws_floats = _kn()._L.load().hulc_grid_bn_bwd_workspace(N, H, W, C) // 4

    def call():
        dz = GridBuf(dev, N, H, W, C, ld=C + pads[3])
        dg_, db_ = out_flat(dev, C, init=base64[0]), out_flat(dev, C, init=base64[1])
        ws = out_flat(dev, ws_floats)
        kn._call("hulc_grid_bn_relu_bwd", bufs[0].t, bufs[0].ld, bufs[1].t, bufs[1].ld, bufs[2].t, bufs[2].ld, bn, N, H, W, C, dz.t, dz.ld, dg_.t, db_.t,
                 int(acc), ws.t, ctr.t if counters else None)
        torch.cuda.synchronize()
        for o, nm in ((dz, "dz"), (dg_, "dgamma"), (db_, "dbeta"), (ws, "workspace"), (ctr, "counters")):
            o.assert_guards(f"{what} {nm}")
        assert not ctr.value().any(), f"{what}: the counters do not read zero after the call"
        return dz.value(), dg_.value().reshape(-1), db_.value().reshape(-1)

    dz, dg_, db_ = call()
    _equal(db_, (s1 + (base64[1] if acc else 0)).float().to(dev), what + " dbeta")
    b0 = base64[0] if acc else 0
    compare(name, "dgamma", dg_, s2 + b0, s2_32.double() + b0, MARGIN["SUM"], grad=True)
    assert not G.borders(dz, N, H, W).float().any(), f"{what}: border rows of dz are not zero"
    compare_rows(name, "dz", dz, dz64, dz32, MARGIN["SUM"])
    dz2, dg2, db2 = call()
    for a, b, nm in ((dz, dz2, "dz"), (dg_, dg2, "dgamma"), (db_, db2, "dbeta")):
        same_bits(a, b, f"{what} {nm}")


# ------------------------------------------------------------------------------------------------
# 5. hulc_grid_upcat_fwd / _bwd
# ------------------------------------------------------------------------------------------------
def _small_map(dev, x_nhwc64, as_grid, pad=0):
    """the small map as a grid tensor's pixels or a dense NHWC map: -> (tensor at pixel (0, 0, 0), (stride n, y, x))"""
    N, Hi, Wi, Cx = x_nhwc64.shape
    if as_grid:
        gb = GridBuf(dev, N, Hi, Wi, Cx, ld=Cx + pad, rows64=G.to_rows(x_nhwc64))
        return gb.px0, gb.strides
    return _in(dev, x_nhwc64, BF), (Hi * Wi * Cx, Wi * Cx, Cx)


@pytest.mark.parametrize("N,Hi,Wi,s,Cx,Cs,fused,x_grid,skip_grid", [
    (2, 3, 4, 2, 64, 32, True, True, False), (2, 5, 5, 1, 128, 64, False, True, True), (3, 2, 3, 4, 64, 0, False, False, False),
    (1, 3, 3, 2, 32, 8, True, False, True), (2, 4, 2, 1, 8, 0, True, True, False), (1, 2, 2, 4, 64, 64, True, False, False)])
def test_grid_upcat_fwd_lattice(dev, N, Hi, Wi, s, Cx, Cs, fused, x_grid, skip_grid):
    """[nearest-up-sampled x * g | skip] on the output grid: x, skip integers, g multiples of 1/4 — exact in bf16; border rows zero"""
    kn = _kn()
    what = f"grid_upcat_fwd {(N, Hi, Wi, s, Cx, Cs)} g={fused} x_grid={x_grid} skip_grid={skip_grid}"
    g = _gen("upfwd", N, Hi, Wi, s, Cx, Cs, fused)
    Ho, Wo = Hi * s, Wi * s
    x64, g64, sk64 = _ints(g, N, Hi, Wi, Cx), _ints(g, N, Cx, lo=-8, hi=8) / 4, _ints(g, N, Ho, Wo, max(Cs, 8))[..., :Cs]
    up = (x64 * g64[:, None, None, :] if fused else x64).repeat_interleave(s, 1).repeat_interleave(s, 2)
    want = G.to_rows(torch.cat([up, sk64], -1))
    assert want.abs().max().item() <= 6 and torch.equal(want, rnd(want, BF))
    xt, xs = _small_map(dev, x64, x_grid, pad=16)
    st, ss = _small_map(dev, sk64.contiguous(), skip_grid, pad=8) if Cs else (None, (0, 0, 0))
    gv = _in(dev, g64) if fused else None
    _row("grid_upcat_fwd")

    def call():
        out = GridBuf(dev, N, Ho, Wo, Cx + Cs)
        kn._call("hulc_grid_upcat_fwd", xt, *xs, gv, st, *ss, N, Ho, Wo, s, Cx, Cs, out.t)
        torch.cuda.synchronize()
        out.assert_guards(what)
        return out.value()

    out = call()
    _equal(out, want.to(BF).to(dev), what)
    same_bits(out, call(), what)


@pytest.mark.parametrize("N,Hi,Wi,s,Cx,fused,x_grid,mode", [
    (2, 3, 4, 2, 64, True, True, "both"), (2, 5, 5, 1, 128, True, False, "both-acc"), (3, 2, 3, 4, 64, False, True, "dsmall"),
    (2, 9, 9, 2, 64, True, True, "dsmall"), (2, 9, 9, 2, 128, True, True, "dg"), (1, 12, 11, 1, 128, False, False, "dsmall")])
def test_grid_upcat_bwd_lattice(dev, N, Hi, Wi, s, Cx, fused, x_grid, mode):
    """dsmall = g * the s x s block sums of dX's first Cx channels (one rounding to bf16), dg (+)= sum over pixels of x * block sums (exact).
    THE BORDER ROWS OF dsmall ARE NOT WRITTEN (include/hulc2_amd.h): the kernel stores the pixel rows only, the sentinel must survive there."""
    kn = _kn()
    what = f"grid_upcat_bwd {(N, Hi, Wi, s, Cx)} g={fused} x_grid={x_grid} {mode}"
    want_small, want_dg, acc = mode in ("both", "both-acc", "dsmall"), mode in ("both", "both-acc", "dg"), mode == "both-acc"
    npt = G.upcat_bwd_npt(N, Cx, Hi, Wi, want_dg)
    if (Hi, Wi) in ((9, 9), (12, 11)) and not want_dg:
        assert npt > 1, f"{what}: the launcher's arithmetic gives one pixel tile"        # the npt > 1 path: dg == NULL and more than 64 pixels
    g = _gen("upbwd", N, Hi, Wi, s, Cx, fused, mode)
    Ho, Wo, Cd = Hi * s, Wi * s, Cx + 32
    d64, x64, g64 = _ints(g, N, Ho, Wo, Cd), _ints(g, N, Hi, Wi, Cx), _ints(g, N, Cx, lo=-8, hi=8) / 4
    bs = d64[..., :Cx].reshape(N, Hi, s, Wi, s, Cx).sum((2, 4))
    small64 = bs * g64[:, None, None, :] if fused else bs
    base64 = _ints(g, N, Cx, lo=-16, hi=16) / 8
    dg64 = (x64 * bs).sum((1, 2)) + (base64 if acc else 0)
    _units((x64 * bs).abs().sum((1, 2)).max().item() + 2, 2.0 ** -3, what + " dg")
    D = GridBuf(dev, N, Ho, Wo, Cd, ld=Cd + 8, rows64=G.to_rows(d64))
    xt, xs = _small_map(dev, x64, x_grid, pad=16)
    gv = _in(dev, g64) if fused else None
    inner = G.interior_mask(N, Hi, Wi).to(dev)
    _row("grid_upcat_bwd" + (" npt>1" if npt > 1 else ""))

    def call():
        ds = GridBuf(dev, N, Hi, Wi, Cx) if want_small else None
        dg_ = Guarded(dev, N, Cx, init=base64) if want_dg else None
        kn._call("hulc_grid_upcat_bwd", D.t, D.ld, xt, *xs, gv, N, Hi, Wi, s, Cx, ds.t if ds else None, dg_.t if dg_ else None, int(acc))
        torch.cuda.synchronize()
        for o, nm in ((ds, "dsmall"), (dg_, "dg")):
            if o is not None:
                o.assert_guards(f"{what} {nm}")
        if ds is not None:
            assert torch.equal(ds.sentinel_rows(), ~inner), f"{what}: the border rows of dsmall are the caller's: the kernel must leave them untouched"
        return (ds.value()[inner] if ds else None), (dg_.value() if dg_ else None)

    ds, dg_ = call()
    if want_small:
        _equal(ds, small64.reshape(-1, Cx).float().to(BF).to(dev), what + " dsmall")
    if want_dg:
        _equal(dg_, dg64.float().to(dev), what + " dg")
    ds2, dg2 = call()
    for a, b, nm in ((ds, ds2, "dsmall"), (dg_, dg2, "dg")):
        if a is not None:
            same_bits(a, b, f"{what} {nm}")


# ------------------------------------------------------------------------------------------------
# 6. the one-channel head, the pixel cross-entropy, hulc_grid_from_nhwc
# ------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(1, 6, 5, 8), (2, 11, 7, 16), (3, 11, 13, 32), (2, 12, 10, 64), (2, 40, 37, 8)]


@pytest.mark.parametrize("N,H,W,C", HEAD_SHAPES, ids=lambda v: str(v))
def test_head_conv_lattice(dev, N, H, W, C):
    """hulc_head_conv_fwd / _dgrad / _wgrad at C = 8, 16, 32, 64: logit0 and dw bit for bit, dx one rounding.  (1, 6, 5, 8): 56 rows, fewer than
    one pass (256 rows) of a weight-gradient workgroup; (3, 11, 13, 32), (2, 12, 10, 64) and (2, 40, 37, 8): more than one workgroup, so the
    fixed-order final sum has several partials"""
    kn = _kn()
    what = f"head_conv {(N, H, W, C)}"
    R, inner = G.grid_R(N, H, W), G.interior_mask(N, H, W)
    nblk, rpp = G.head_wgrad_blocks(R, C)
    if (N, H, W, C) == (1, 6, 5, 8):
        assert R < rpp
    if C >= 32 or H == 40:
        assert nblk > 1, f"{what}: the launcher's arithmetic gives one workgroup"
    g = _gen("head", N, H, W, C)
    x64, w64, b64 = _ints(g, N, C, H, W), _ints(g, 1, C, 3, 3) / 8, _ints(g, 1, lo=-16, hi=16) / 8
    gr64 = G.to_rows(_ints(g, N, H, W, 1)).reshape(-1)                       # d logit per grid row, zero on the border rows
    base64 = _ints(g, C * 9, lo=-16, hi=16) / 8
    xr = x64.clone().requires_grad_(True)
    wr = w64.clone().requires_grad_(True)
    lg = F.conv2d(xr, wr, b64, padding=1)
    lg.backward(G.from_rows(gr64[:, None], N, H, W).permute(0, 3, 1, 2))
    logit64 = G.to_rows(_nhwc(lg.detach())).reshape(-1)
    _units(9 * C * 9 / 8 + 2, 2.0 ** -3, what + " logit0")
    _units(N * H * W * 9 + 2, 2.0 ** -3, what + " dw")
    X = GridBuf(dev, N, H, W, C, ld=C + (8 if C != 32 else 0), rows64=G.to_rows(_nhwc(x64)))
    w, b, gr = _in(dev, w64), _in(dev, b64), _in(dev, gr64)
    ws_floats = kn._L.load().hulc_head_conv_wgrad_workspace(N, H, W, C) // 4
    for k in ("head_conv_fwd", "head_conv_dgrad", "head_conv_wgrad"):
        _row(f"{k} C={C}")

    def call():
        o0, dx = out_flat(dev, R), GridBuf(dev, N, H, W, C, ld=C + 8)
        dw, dwa, ws = out_flat(dev, C * 9), out_flat(dev, C * 9, init=base64), out_flat(dev, ws_floats)
        kn._call("hulc_head_conv_fwd", X.t, X.ld, w, b, N, H, W, C, o0.t)
        kn._call("hulc_head_conv_dgrad", gr, w, N, H, W, C, dx.t, dx.ld)
        kn._call("hulc_head_conv_wgrad", X.t, X.ld, gr, N, H, W, C, dw.t, 0, ws.t)
        kn._call("hulc_head_conv_wgrad", X.t, X.ld, gr, N, H, W, C, dwa.t, 1, ws.t)
        torch.cuda.synchronize()
        for o, nm in ((o0, "logit0"), (dx, "dx"), (dw, "dw"), (dwa, "dw (accumulate)"), (ws, "workspace")):
            o.assert_guards(f"{what} {nm}")
        return o0.value().reshape(-1), dx.value(), dw.value().reshape(-1), dwa.value().reshape(-1)

    outs = call()
    _equal(outs[0], logit64.float().to(dev), what + " logit0")
    _equal(outs[1], G.to_rows(_nhwc(xr.grad)).float().to(BF).to(dev), what + " dx")
    _equal(outs[2], wr.grad.reshape(-1).float().to(dev), what + " dw")
    _equal(outs[3], (wr.grad.reshape(-1) + base64).float().to(dev), what + " dw (accumulate)")
    for a, b_, nm in zip(outs, call(), ("logit0", "dx", "dw", "dw (accumulate)")):
        same_bits(a, b_, f"{what} {nm}")


@pytest.mark.parametrize("N,H,W,C", [(4, 5, 7, 8), (4, 33, 35, 32), (5, 40, 37, 16)], ids=lambda v: str(v))
def test_pixel_cross_entropy(dev, N, H, W, C):
    """hulc_pixel_ce_fwd / _bwd / _bwd_rows against float64 log_softmax: H W = 35 (< 64) and 1155 / 1480 (not multiples of the 1024 threads),
    p0 at the four corners, logits spanning about +-30 (softmax without the max subtracted would lose every small term); the backward kernels
    get the float64 lse rounded to fp32, not the forward kernel's"""
    kn = _kn()
    what = f"pixel_ce {(N, H, W, C)}"
    g = _gen("ce", N, H, W)
    inner = G.interior_mask(N, H, W)
    lg64 = rnd(_uni(g, N, H, W, 1) * 30, F32)
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 3)]
    p0 = torch.tensor([corners[n % 5] for n in range(N)], dtype=torch.int64)
    up64 = rnd(torch.tensor([0.7], dtype=torch.float64), F32)
    onehot = torch.zeros(N, H, W, dtype=torch.float64)
    onehot[torch.arange(N), p0[:, 0], p0[:, 1]] = 1

    def ref(dt):
        flat = lg64.reshape(N, -1).to(dt)
        lse = torch.logsumexp(flat, 1)
        return lse, flat[torch.arange(N), p0[:, 0] * W + p0[:, 1]]

    lse64, picked64 = ref(torch.float64)
    lse32, _ = ref(torch.float32)
    lse_in = rnd(lse64, F32)

    def ref_bwd(dt):
        d = torch.exp(lg64.reshape(N, H, W).to(dt) - lse_in.to(dt)[:, None, None]) - onehot.to(dt)
        return G.to_rows((d * (up64.to(dt) / torch.tensor(float(N * H * W), dtype=dt)))[..., None]).reshape(-1)

    d64, d32 = ref_bwd(torch.float64), ref_bwd(torch.float32)
    logit0 = _in(dev, G.to_rows(lg64).reshape(-1))
    p0d, lse_d, up = _in(dev, p0.double(), I32), _in(dev, lse_in), _in(dev, up64)
    R = G.grid_R(N, H, W)

    def call():
        lse, picked, rows, dz = out_flat(dev, N), out_flat(dev, N), out_flat(dev, R), GridBuf(dev, N, H, W, C)
        kn._call("hulc_pixel_ce_fwd", logit0, p0d, N, H, W, lse.t, picked.t)
        kn._call("hulc_pixel_ce_bwd_rows", logit0, p0d, lse_d, up, N, H, W, rows.t)
        kn._call("hulc_pixel_ce_bwd", logit0, p0d, lse_d, up, N, H, W, C, dz.t)
        torch.cuda.synchronize()
        for o, nm in ((lse, "lse"), (picked, "picked"), (rows, "rows"), (dz, "dz")):
            o.assert_guards(f"{what} {nm}")
        return lse.value().reshape(-1), picked.value().reshape(-1), rows.value().reshape(-1), dz.value()

    lse, picked, rows, dz = call()
    compare("pixel_ce_fwd", "lse", lse, lse64, lse32, MARGIN["SUM"])
    _equal(picked, picked64.float().to(dev), what + " picked")
    assert not rows[~inner.to(dev)].any() and not G.borders(dz, N, H, W).float().any(), f"{what}: border rows are not zero"
    assert not dz[:, 1:].float().any(), f"{what}: channels 1 .. C - 1 of dz are not zero"
    compare("pixel_ce_bwd_rows", "g", rows, d64, d32, MARGIN["SUM"])
    compare("pixel_ce_bwd", "dz[:, 0]", dz[:, 0], d64, d32, MARGIN["SUM"], out_dtype=BF)
    for a, b, nm in zip((lse, picked, rows, dz), call(), ("lse", "picked", "rows", "dz")):
        same_bits(a, b, f"{what} {nm}")


@pytest.mark.parametrize("N,H,W,C,pad", [(2, 5, 7, 8, 8), (3, 4, 3, 96, 0), (1, 9, 9, 64, 32)])
def test_grid_from_nhwc_exact(dev, N, H, W, C, pad):
    kn = _kn()
    what = f"grid_from_nhwc {(N, H, W, C)} ldy={C + pad}"
    x64 = rnd(_uni(_gen("nhwc", N, H, W, C), N, H, W, C) * 4, BF)
    x = _in(dev, x64, BF)
    _row("grid_from_nhwc")

    def call():
        y = GridBuf(dev, N, H, W, C, ld=C + pad)
        kn._call("hulc_grid_from_nhwc", x, N, H, W, C, y.t, y.ld)
        torch.cuda.synchronize()
        y.assert_guards(what)
        return y.value()

    y = call()
    _equal(y, G.to_rows(x64).to(BF).to(dev), what)
    same_bits(y, call(), what)


# ------------------------------------------------------------------------------------------------
# 7. hulc_depth_nll_fwd / _bwd
# ------------------------------------------------------------------------------------------------
def _depth_inputs(B, D):
    g = _gen("depth", B, D)
    x = rnd(torch.randn(B, D, generator=g, dtype=torch.float64), F32)
    w_mu, b_mu = rnd(torch.randn(D, generator=g, dtype=torch.float64) / D ** 0.5, F32), rnd(torch.randn(1, generator=g, dtype=torch.float64), F32)
    w_s, b_s = rnd(torch.randn(D, generator=g, dtype=torch.float64) * (10.0 / D ** 0.5), F32), torch.tensor([-6.0], dtype=torch.float64)
    t = rnd(torch.randn(B, generator=g, dtype=torch.float64), F32)
    return x, w_mu, b_mu, w_s, b_s, t


def _depth_fwd(x, w_mu, b_mu, w_s, b_s, t, dt):
    """depth_gaussian.py:67-69,94-102: the two heads, sigma = exp(clamp(log_sigma, -20, 2)), GaussianNLLLoss with sigma as the variance"""
    x, w_mu, b_mu, w_s, b_s, t = (v.to(dt) for v in (x, w_mu, b_mu, w_s, b_s, t))
    mu, ls = x @ w_mu + b_mu, x @ w_s + b_s
    sg = torch.exp(ls.clamp(-20, 2))
    var = sg.clamp_min(torch.tensor(1e-6, dtype=torch.float32).to(dt))
    return mu, sg, ls, (0.5 * (torch.log(var) + (mu - t) ** 2 / var)).mean()


DEPTH_SHAPES = [(32, 256), (3, 256), (70, 96), (1, 40), (4096, 72)]


@pytest.mark.parametrize("B,D", DEPTH_SHAPES)
def test_depth_nll_fwd(dev, B, D):
    kn = _kn()
    what = f"depth_nll_fwd B={B} D={D}"
    ins = _depth_inputs(B, D)
    r64, r32 = _depth_fwd(*ins, torch.float64), _depth_fwd(*ins, torch.float32)
    if B >= 32:
        ls = r64[2]
        assert (ls > 2).any() and (ls < -13.9).any() and (ls < -20).any(), f"{what}: the clamp ranges the case is about are not entered"
    d_in = [_in(dev, v) for v in ins]

    def call():
        outs = [out_flat(dev, B), out_flat(dev, B), out_flat(dev, B), out_flat(dev, 1)]
        kn._call("hulc_depth_nll_fwd", d_in[0], B, D, *d_in[1:], *[o.t for o in outs])
        torch.cuda.synchronize()
        for o, nm in zip(outs, ("mu", "sigma", "log_sigma", "loss")):
            o.assert_guards(f"{what} {nm}")
        return [o.value().reshape(-1) for o in outs]

    got = call()
    for v, a, b, nm in zip(got, r64, r32, ("mu", "sigma", "log_sigma", "loss")):
        compare("depth_nll_fwd", nm, v, a.reshape(-1), b.reshape(-1), MARGIN["SEQ" if nm == "loss" and B > 1024 else "SUM"])
    for a, b, nm in zip(got, call(), ("mu", "sigma", "log_sigma", "loss")):
        same_bits(a, b, f"{what} {nm}")


# every shape with nothing and with everything accumulated; each bit on its own at the clamp-range shape, B = 1 and the ragged D
DEPTH_BWD = [(B, D, m, True) for B, D in DEPTH_SHAPES for m in (0, 15)] + [(B, D, m, dx) for B, D in ((32, 256), (1, 40), (70, 96))
                                                                             for m, dx in ((1, True), (2, False), (4, True), (8, False))]


@pytest.mark.parametrize("B,D,mask,with_dx", DEPTH_BWD)
def test_depth_nll_bwd(dev, B, D, mask, with_dx):
    """mu, sigma and log_sigma are inputs of the backward: the float64 forward rounded to fp32.  Each bit of accumulate_mask on its own (1: dw_mu,
    2: db_mu, 4: dw_sigma, 8: db_sigma), none, all; dx == NULL"""
    kn = _kn()
    what = f"depth_nll_bwd B={B} D={D} mask={mask} dx={with_dx}"
    x, w_mu, b_mu, w_s, b_s, t = _depth_inputs(B, D)
    mu, sg, ls, _ = (rnd(v, F32) for v in _depth_fwd(x, w_mu, b_mu, w_s, b_s, t, torch.float64))
    gout = rnd(torch.tensor([0.9], dtype=torch.float64), F32)
    g = _gen("depthbase", B, D)
    bases = [rnd(_uni(g, n), F32) for n in (D, 1, D, 1)]

    def ref(dt):
        x_, wm, wsg, mu_, sg_, ls_, t_, go = (v.to(dt) for v in (x, w_mu, w_s, mu, sg, ls, t, gout))
        floor = torch.tensor(1e-6, dtype=torch.float32).to(dt)
        gg = go / B
        var, r = sg_.clamp_min(floor), mu_ - t_
        dvar = gg * 0.5 * (1 / var - r * r / (var * var))
        dm = gg * r / var
        dl = torch.where((sg_ >= floor) & (ls_ >= -20) & (ls_ <= 2), dvar * sg_, torch.zeros((), dtype=dt))
        outs = [dm @ x_, dm.sum().reshape(1), dl @ x_, dl.sum().reshape(1)]
        outs = [o + (b.to(dt) if mask >> i & 1 else 0) for i, (o, b) in enumerate(zip(outs, bases))]
        return [dm[:, None] * wm[None, :] + dl[:, None] * wsg[None, :]] + outs

    r64, r32 = ref(torch.float64), ref(torch.float32)
    d_in = [_in(dev, v) for v in (x, w_mu, w_s, mu, sg, ls, t, gout)]

    def call():
        dx = Guarded(dev, B, D) if with_dx else None
        outs = [out_flat(dev, b.numel(), init=b) for b in bases]
        kn._call("hulc_depth_nll_bwd", d_in[0], B, D, *d_in[1:], dx.t if with_dx else None, *[o.t for o in outs], mask)
        torch.cuda.synchronize()
        for o, nm in zip([dx] + outs, ("dx", "dw_mu", "db_mu", "dw_sigma", "db_sigma")):
            if o is not None:
                o.assert_guards(f"{what} {nm}")
        return [dx.value() if with_dx else None] + [o.value().reshape(-1) for o in outs]

    got = call()
    for v, a, b, nm in zip(got, r64, r32, ("dx", "dw_mu", "db_mu", "dw_sigma", "db_sigma")):
        if v is not None:
            compare("depth_nll_bwd", nm, v, a, b, MARGIN["SUM"], grad=True)
    for a, b, nm in zip(got, call(), ("dx", "dw_mu", "db_mu", "dw_sigma", "db_sigma")):
        if a is not None:
            same_bits(a, b, f"{what} {nm}")


# ------------------------------------------------------------------------------------------------
# 8. refusals: the launcher's own message, sentinel outputs untouched, no path reported
# ------------------------------------------------------------------------------------------------
def test_gridconv_refusals(dev):
    kn = _kn()
    N, H, W = 1, 4, 3
    R = G.grid_R(N, H, W)
    g = _gen("refuse")

    def attempt(message, Cin=32, Cout=32, ldx=None, lead_x=0, lead_w=0, x_null=False, y_null=False, o_null=True, fused=False, ldadd=None):
        x = GridBuf(dev, N, H, W, max(Cin, 32), ld=(max(ldx or 0, Cin, 32) + 15) // 8 * 8, rows64=G.to_rows(_ints(g, N, H, W, max(Cin, 32))), lead=lead_x)
        wt = _in(dev, _ints(g, Cout, 9 * Cin) / 8, BF, lead=lead_w)
        y, o0, st = GridBuf(dev, N, H, W, Cout), out_flat(dev, R), Guarded(dev, 2, Cout)
        add = GridBuf(dev, N, H, W, Cout, rows64=G.to_rows(_ints(g, N, H, W, Cout)))
        ldx_ = Cin if ldx is None else ldx
        if fused:
            c = lambda: kn._call("hulc_gridconv3x3_fused", x.t, ldx_, wt, None if y_null else y.t, y.ld, N, H, W, Cin, Cout, None, add.t, add.ld if ldadd is None else ldadd, 1)
        else:
            c = lambda: kn._call("hulc_gridconv3x3", None if x_null else x.t, ldx_, wt, None if y_null else y.t, y.ld, N, H, W, Cin, Cout, 0, st.t,
                                 None if o_null else o0.t, None)
        refused(c, message, y, o0, st)
        assert kn.conv_last_path() == ("", {}), f"a refused call reports the path {kn.conv_last_path()}"

    multiple, aligned, null = ("hulc_gridconv3x3: Cin and Cout must be positive multiples of 32", "hulc_gridconv3x3: rows must be 16-byte aligned",
                               "hulc_gridconv3x3: null pointer")
    attempt(multiple, Cin=48)
    attempt(multiple, Cout=48)
    attempt(aligned, ldx=36)                                     # ldx % 8
    attempt(aligned, Cin=64, ldx=32)                             # ldx < Cin
    attempt(aligned, lead_x=1)                                   # x two bytes off
    attempt(aligned, lead_w=1)                                   # wt two bytes off
    attempt(null, x_null=True)
    attempt(null, y_null=True, o_null=True)
    attempt("hulc_gridconv3x3_fused: null pointer", fused=True, y_null=True)
    attempt("hulc_gridconv3x3_fused: residual rows shorter than Cout", fused=True, ldadd=24)


def test_affordance_refusals(dev):
    kn = _kn()
    g = _gen("refuse2")
    N, Hi, Wi, s, Cx = 1, 2, 2, 2, 64
    x, xs = _small_map(dev, _ints(g, N, Hi, Wi, Cx), False)
    out = GridBuf(dev, N, 5, 4, Cx + 8)
    refused(lambda: kn._call("hulc_grid_upcat_fwd", x, *xs, None, None, 0, 0, 0, N, 5, 4, s, Cx, 0, out.t), "hulc_grid_upcat_fwd: bad argument", out)      # Ho % s
    refused(lambda: kn._call("hulc_grid_upcat_fwd", x, *xs, None, None, 0, 0, 0, N, 4, 4, s, Cx, 8, out.t), "hulc_grid_upcat_fwd: bad argument", out)      # Cs, no skip
    D = GridBuf(dev, N, 4, 4, 32, rows64=G.to_rows(_ints(g, N, 4, 4, 32)))
    ds, dg_ = GridBuf(dev, N, Hi, Wi, 32), out_flat(dev, 32)
    refused(lambda: kn._call("hulc_grid_upcat_bwd", D.t, D.ld, x, *xs, None, N, Hi, Wi, s, 32, ds.t, dg_.t, 0),
            "hulc_grid_upcat_bwd: bad argument (Cx must be a multiple of 64)", ds, dg_)
    for C in (24, 128):
        H, W = 3, 3
        R = G.grid_R(1, H, W)
        X = GridBuf(dev, 1, H, W, C, rows64=G.to_rows(_ints(g, 1, H, W, C)))
        w, b, gr = _in(dev, _ints(g, C * 9) / 8), _in(dev, _ints(g, 1)), _in(dev, _ints(g, R))
        o0, dx, dw, ws = out_flat(dev, R), GridBuf(dev, 1, H, W, C), out_flat(dev, C * 9), out_flat(dev, 9 * C * 4)
        msg = "hulc_head_conv: C must be 8, 16, 32 or 64"
        refused(lambda: kn._call("hulc_head_conv_fwd", X.t, X.ld, w, b, 1, H, W, C, o0.t), msg, o0)
        refused(lambda: kn._call("hulc_head_conv_dgrad", gr, w, 1, H, W, C, dx.t, dx.ld), msg, dx)
        refused(lambda: kn._call("hulc_head_conv_wgrad", X.t, X.ld, gr, 1, H, W, C, dw.t, 0, ws.t), msg, dw, ws)
    C = 32
    part, ga, be, bn = _in(dev, _ints(g, 3, 2, C)), _in(dev, _ints(g, C)), _in(dev, _ints(g, C)), Guarded(dev, 4, C)
    refused(lambda: kn._call("hulc_grid_bn_finalize", part, 3, C, 1, ga, be, 1e-5, 0.1, bn.t, None, None, None, None), "hulc_grid_bn_finalize: bad argument", bn)
    B, Dd = 4097, 8
    ins = [_in(dev, _uni(g, *sh)) for sh in ((B, Dd), (Dd,), (Dd,), (B,), (B,), (B,), (B,), (1,))]
    outs = [Guarded(dev, B, Dd)] + [out_flat(dev, n) for n in (Dd, 1, Dd, 1)]
    refused(lambda: kn._call("hulc_depth_nll_bwd", ins[0], B, Dd, *ins[1:], *[o.t for o in outs], 0), "hulc_depth_nll_bwd: 1 <= B <= 4096", *outs)
    xn = _in(dev, _ints(g, 1, 3, 3, 16), BF)
    y = GridBuf(dev, 1, 3, 3, 16)
    refused(lambda: kn._call("hulc_grid_from_nhwc", xn, 1, 3, 3, 16, y.t, 8), "hulc_grid_from_nhwc: bad argument", y)
