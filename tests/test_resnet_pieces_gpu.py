"""Kernel-level tests of the frozen ResNet trunk's pieces that are not plain convolutions: csrc/resnet.hip (BatchNorm on batch statistics, forward
and backward; max pool, forward and backward; the zero-inserting scatter; both input normalisations) and the packed 7 x 4 "double pixel" stem
hulc_r3m_stem_fwd of csrc/conv.hip, each against a few lines of float64 torch.  The pattern of a case and the tolerance rule are in
tests/kcheck.py; what is particular to this file:

EXACT cases.  The max pool (both directions), the scatter and the stem on a {-1, 0, 1} lattice have results that fp32 holds exactly whatever the
order of the sums, so they are asserted with `torch.equal` against the float64 reference (rounded once to a bf16 output).  The max pool's inputs
are post-ReLU lattices — four values, half of the elements exact zeros, the largest value the commonest of the rest — so that most windows
have ties and "first maximum in (kh, kw) scan order" is the rule under test, not the values.

SHAPES are chosen for the thread layouts of the BatchNorm statistics kernels (8 channels per thread, 256 / (C / 8) row lanes, slices of 256
rows, two rows in flight per lane), not for the workload: see BN_C / BN_M."""
import pytest
import torch
import torch.nn.functional as F

from tests import kcheck as K
from tests.kcheck import compare, out_flat, refused, rnd, same_bits

pytestmark = pytest.mark.gpu

# Margins of margin * max(e_ref, 2^-23), e_ref = the float32 CPU evaluation of the same formula against float64 (tests/kcheck.py).
#   SUM 4: the class of tests/test_reductions_gpu.py.  None of these kernels uses a fast intrinsic: the BatchNorm statistics are fp32 lane sums
#          finished in double (sqrt and division in double), everything else is float32 sums, products and copies, so only the order of the
#          sums and the places of the roundings differ from the CPU's.
# A kernel that cannot meet 4 is a finding and gets a row here with the measured float32-CPU and GPU errors and the cause.
#   kernel                        what     cpu-f32     gpu        cause
#   (none)
MARGIN = {"SUM": 4.0}

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    K.report("tests/test_resnet_pieces_gpu.py")


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


def _ints(g, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _in(dev, t64, dtype, lead=0):
    """an input tensor inside a NaN-sentinel allocation (`lead` elements in: a view that is not 16-byte aligned): a stray read that is consumed
    surfaces as a non-finite output"""
    return out_flat(dev, t64.numel(), dtype, init=t64, lead=lead).t.reshape(t64.shape)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _equal(got, ref64, dtype, what):
    want = ref64.float().to(dtype)                       # (the exact value fits fp32: one rounding to a low-precision output)
    got = got.cpu()
    assert got.dtype == dtype and got.shape == want.shape and torch.equal(got, want), (
        f"{what}: {(got != want).sum().item()} of {got.numel()} elements differ from the float64 reference "
        f"(max abs difference {(got.double() - want.double()).abs().max().item():.3e}, non-finite {(~torch.isfinite(got.float())).sum().item()})")


# ------------------------------------------------------------------------------------------------
# BatchNorm on batch statistics, forward (hulc_nhwc_bn_train_fwd_saved)
# ------------------------------------------------------------------------------------------------
# C: 8 = 256 row lanes per chunk column; 64 = 32; 256 = 8; 384 = 5 row lanes of 48 threads, 16 threads of the workgroup idle; 512 = 4;
#    2048 = one row lane, every thread its own chunk
# M: 1 = a single row (variance 0); 3 = fewer rows than row lanes; 255 / 256 = one slice, ragged and full; 257 = two slices of 129 and 128 rows;
#    1000 = four slices of 250 rows (an odd number of rows per lane wherever 250 / RL is odd or ragged: the two-rows-in-flight loop's tail runs)
BN_C = (8, 64, 256, 384, 512, 2048)
BN_M = (1, 3, 255, 256, 257, 1000)
EPS = 1e-5


def _bn_options(i):
    """the options of case i, cycled with coprime periods so that the (C, M) grid meets every value of every option"""
    return dict(add=(None, "y", "bf16")[i % 3], relu=bool(i % 2), ydt=BF if i % 4 == 1 else F32, momentum=1.0 if i % 5 == 3 else 0.1,
                running=i % 7 != 4)


def _bn_data(g, M, C, mu=None, zdt=F32):
    """z with per-channel spreads in [0.5, 2] and means in [-2, 2]; `mu`: z ~ N(mu + a per-channel jitter, 1) instead"""
    if mu is None:
        z = _randn(g, M, C) * (0.5 + 1.5 * _rand(g, C)) + (4.0 * _rand(g, C) - 2.0)
    else:
        z = _randn(g, M, C) + (mu + 0.5 * _randn(g, C))
    return (rnd(z, zdt), rnd(0.5 + _rand(g, C), F32), rnd(_randn(g, C), F32), rnd(_randn(g, C), F32), rnd(0.5 + _rand(g, C), F32))


def _bn_fwd_ref(z, gamma, beta, rm, rv, add, relu, momentum, dt):
    """(y, mean, rstd, running_mean, running_var) of nn.BatchNorm2d in training mode over the rows of z, evaluated in `dt` on the CPU.
    float32: the statistics are torch's own (native_batch_norm, what F.batch_norm calls), y is the kernel's formula z * scale + shift on them.
    A single row: torch refuses it (F.batch_norm) or returns NaN for running_var (the factor M / (M - 1)); the kernel keeps the biased variance
    0 there, which is what this reference states for M = 1."""
    M = z.shape[0]
    z, gamma, beta, rm, rv = (t.to(dt) for t in (z, gamma, beta, rm, rv))
    if dt == torch.float32 and M > 1:
        rm, rv = rm.clone(), rv.clone()
        _, mean, rstd = torch.native_batch_norm(z, gamma, beta, rm, rv, True, momentum, EPS)
    else:
        mean = z.mean(0)
        var = ((z - mean) ** 2).mean(0)
        rstd = 1.0 / torch.sqrt(var + EPS)
        rm = (1.0 - momentum) * rm + momentum * mean
        rv = (1.0 - momentum) * rv + momentum * (var * M / (M - 1) if M > 1 else var)
    if dt == torch.float32:
        scale = gamma * rstd
        y = z * scale + (beta - mean * scale)
    else:
        y = (z - mean) * rstd * gamma + beta
    if add is not None:
        y = y + add.to(dt)
    return (torch.relu(y) if relu else y), mean, rstd, rm, rv


def _bn_fwd_case(dev, C, M, add, relu, ydt, momentum, running, mu=None, zdt=F32, kernel="nhwc_bn_train_fwd"):
    from hulc2_amd import kernels as kn

    what = f"bn fwd C={C} M={M} add={add} relu={relu} y={ydt} mom={momentum} running={running} mu={mu} z={zdt}"
    g = _gen("bnf", C, M, add, relu, str(ydt), momentum, running, mu, str(zdt))
    z64, ga64, be64, rm64, rv64 = _bn_data(g, M, C, mu, zdt)
    adt = None if add is None else (ydt if add == "y" else BF)
    a64 = None if add is None else rnd(_randn(g, M, C), adt)
    z, ga, be = _in(dev, z64, zdt), _in(dev, ga64, F32), _in(dev, be64, F32)
    a = None if add is None else _in(dev, a64, adt)
    r64 = _bn_fwd_ref(z64, ga64, be64, rm64, rv64, a64, relu, momentum, torch.float64)
    r32 = _bn_fwd_ref(z64, ga64, be64, rm64, rv64, a64, relu, momentum, torch.float32)

    def call():
        y, sv = out_flat(dev, M * C, ydt), out_flat(dev, 2 * C, F32)
        rm, rv = (out_flat(dev, C, F32, init=t) if running else None for t in (rm64, rv64))
        kn.nhwc_bn_train_fwd(z, M, C, ga, be, EPS, momentum, rm.t if running else None, rv.t if running else None, y.t.reshape(M, C), add=a, relu=relu,
                             saved=sv.t.reshape(2, C))
        torch.cuda.synchronize()
        for o, nm in ((y, "y"), (sv, "saved"), (rm, "running_mean"), (rv, "running_var")):
            if o is not None:
                o.assert_guards(f"{what} {nm}")
        return [y.value().reshape(M, C), sv.value().reshape(2, C)[0], sv.value().reshape(2, C)[1]] + ([rm.value(), rv.value()] if running else [])

    got = call()
    names = ("y", "mean", "rstd", "run_mean", "run_var")
    for i in list(range(1, len(got))) + [0]:             # the statistics first: a wrong one is named before the y it spoils
        compare(kernel, names[i], got[i], r64[i], r32[i], MARGIN["SUM"], out_dtype=ydt if i == 0 else F32)
    for v, w, nm in zip(got, call(), names):
        same_bits(v, w, f"{what} {nm}")
    return got


@pytest.mark.parametrize("C", BN_C)
@pytest.mark.parametrize("M", BN_M)
def test_bn_train_fwd(dev, C, M):
    _bn_fwd_case(dev, C, M, **_bn_options(BN_C.index(C) * len(BN_M) + BN_M.index(M)))


def test_bn_train_fwd_options_cover_everything():
    """the cycled options of the grid above meet every value the issue lists (a guard against an edit of BN_C / BN_M that loses one)"""
    opts = [_bn_options(i) for i in range(len(BN_C) * len(BN_M))]
    for key, values in (("add", (None, "y", "bf16")), ("relu", (False, True)), ("ydt", (BF, F32)), ("momentum", (0.1, 1.0)), ("running", (False, True))):
        assert {o[key] for o in opts} == set(values), key
    assert any(o["add"] == "bf16" and o["ydt"] == F32 for o in opts), "a bf16 residual under an fp32 output"


def test_bn_train_fwd_capped_slices(dev):
    """M > 262,144: the slice count is capped at 1024, so a slice holds more than 256 rows (257 here) and a row lane of the C = 8 layout two"""
    _bn_fwd_case(dev, 8, 262400, None, True, F32, 0.1, True)


def test_bn_train_fwd_bf16_map(dev):
    """a bf16 z (one 16-byte load per chunk instead of two), bf16 residual and output"""
    _bn_fwd_case(dev, 64, 257, "y", True, BF, 0.1, True, zdt=BF)


@pytest.mark.parametrize("mu", (16.0, 64.0))
def test_bn_train_fwd_offset_mean(dev, mu):
    """z ~ N(mu, 1): the variance must not be formed from raw fp32 sums of z and z^2, whose difference cancels (mean / std)^2 of their digits
    (4e-4 relative at mu = 64 by the CPU emulation of such sums; torch's float32 CPU BatchNorm stays at 1e-7).  The bound is the one of every
    other case: MARGIN * max(e_ref, 2^-23)."""
    _bn_fwd_case(dev, 64, 8192, None, False, F32, 0.1, True, mu=mu, kernel="nhwc_bn_train_fwd offset")


def test_bn_train_fwd_refusals(dev):
    from hulc2_amd import kernels as kn

    g = _gen("bn refusals")

    def attempt(C, M, message, lead=0, rows=4):
        z = _in(dev, _randn(g, rows, C), F32, lead=lead)
        ga, be = _in(dev, _rand(g, C), F32), _in(dev, _rand(g, C), F32)
        y, sv = out_flat(dev, rows * C, F32), out_flat(dev, 2 * C, F32)
        rm, rv = out_flat(dev, C, F32, init=_randn(g, C)), out_flat(dev, C, F32, init=_rand(g, C))
        refused(lambda: kn.nhwc_bn_train_fwd(z, M, C, ga, be, EPS, 0.1, rm.t, rv.t, y.t.reshape(rows, C), saved=sv.t.reshape(2, C)), message, y, sv, rm, rv)

    shape = "hulc_nhwc_bn_train_fwd: C must be a multiple of 8 (a divisor of 256 below 256)"
    attempt(24, 4, shape)                  # a multiple of 8 that does not divide 256: the row lanes would not tile the workgroup
    attempt(12, 4, shape)
    attempt(2056, 4, shape)                # more than 256 chunks: the statistics kernel's chunk loop is not what the workspace is sized for
    attempt(64, 0, shape)
    attempt(64, 4, "hulc_nhwc_bn_train_fwd: 16-byte aligned rows", lead=1)       # a view 4 bytes in


# ------------------------------------------------------------------------------------------------
# BatchNorm backward (hulc_nhwc_bn_train_bwd)
# ------------------------------------------------------------------------------------------------
def _bn_bwd_ref(dy, y, z, gamma, mean, rstd, base_g, base_b, dt):
    """the formula of the kernel's header comment in `dt`: g = dy * (y > 0) or dy; s1 = sum g, s2 = sum g * xhat, xhat = (z - mean) * rstd;
    dz = gamma * rstd * (g - s1 / M - xhat * s2 / M); dgamma = s2, dbeta = s1 (on top of base_g / base_b when accumulating)"""
    M = z.shape[0]
    dy, z, gamma, mean, rstd = (t.to(dt) for t in (dy, z, gamma, mean, rstd))
    g = dy if y is None else torch.where(y > 0, dy, torch.zeros_like(dy))
    xhat = (z - mean) * rstd
    s1, s2 = g.sum(0), (g * xhat).sum(0)
    dz = gamma * rstd * (g - s1 / M - xhat * (s2 / M))
    return dz, g, s2 + (0 if base_g is None else base_g.to(dt)), s1 + (0 if base_b is None else base_b.to(dt))


# C, M, dy / y type, dz / g_out type, y given, g_out given, parameter gradients: None | "write" | "accumulate"
BN_BWD = [
    (8, 3, F32, F32, True, True, "write"),
    (8, 257, BF, BF, True, True, "accumulate"),
    (8, 1000, BF, F32, False, False, None),
    (384, 3, BF, BF, False, True, "accumulate"),
    (384, 257, F32, F32, True, False, "write"),
    (384, 1000, BF, BF, True, True, "write"),
    (2048, 3, BF, F32, True, True, None),
    (2048, 257, F32, BF, False, True, "write"),
    (2048, 1000, F32, F32, True, True, "accumulate"),
    (64, 256, BF, BF, True, True, "write"),
    (512, 255, F32, F32, False, True, "accumulate"),
]


def _bn_bwd_inputs(g, C, M, gdt, with_y):
    """dy with a per-channel mean that is large against its spread (g - mean(g) is the cancelling term: a wrong sums[] shows); y = the forward's
    ReLU output rounded to the storage type, with exact zeros and, on every third of them, negative zeros"""
    z64, ga64, be64, _, _ = _bn_data(g, M, C)
    dy64 = rnd((1.0 + 2.0 * _rand(g, C)) * torch.where(_rand(g, C) < 0.5, -1.0, 1.0) + 0.05 * _randn(g, M, C), gdt)
    mean64 = z64.mean(0)
    rstd64 = 1.0 / torch.sqrt(((z64 - mean64) ** 2).mean(0) + EPS)
    y64 = None
    if with_y:
        y64 = rnd(torch.relu((z64 - mean64) * rstd64 * ga64 + be64), gdt)
        zeros = (y64 == 0).reshape(-1).nonzero().reshape(-1)[::3]
        y64.reshape(-1)[zeros] = -0.0
        assert M * C < 64 or (len(zeros) > 0 and (y64 > 0).any()), "the case needs both sides of the mask"
    return z64, ga64, be64, dy64, y64, mean64, rstd64


def _bn_bwd_call(dev, kn, what, M, C, dy, y, z, ga, saved, odt, with_gout, params, bg64, bb64):
    dz = out_flat(dev, M * C, odt)
    go = out_flat(dev, M * C, odt) if with_gout else None
    dg, db = (out_flat(dev, C, F32, init=t if params == "accumulate" else None) if params else None for t in (bg64, bb64))
    kn.nhwc_bn_train_bwd(dy, y, z, M, C, ga, saved, dz.t.reshape(M, C), g_out=go.t.reshape(M, C) if with_gout else None,
                         dgamma=dg.t.reshape(C) if params else None, dbeta=db.t.reshape(C) if params else None, accumulate_params=params == "accumulate")
    torch.cuda.synchronize()
    for o, nm in ((dz, "dz"), (go, "g_out"), (dg, "dgamma"), (db, "dbeta")):
        if o is not None:
            o.assert_guards(f"{what} {nm}")
    return [o.value().reshape(-1) if o is not None else None for o in (dz, go, dg, db)]


def _bn_bwd_check(kernel, what, got, again, r64, r32, gdt, odt):
    dz, go, dg, db = got
    compare(kernel, "dz", dz, r64[0], r32[0], MARGIN["SUM"], grad=True, out_dtype=odt)
    if go is not None:                                   # the masked incoming gradient is a copy: exact (rounded once where dy is fp32 and g_out bf16)
        _equal(go, r64[1].reshape(-1), odt, f"{what} g_out")
    if dg is not None:
        compare(kernel, "dgamma", dg, r64[2], r32[2], MARGIN["SUM"], grad=True)
        compare(kernel, "dbeta", db, r64[3], r32[3], MARGIN["SUM"], grad=True)
    for v, w, nm in zip(got, again, ("dz", "g_out", "dgamma", "dbeta")):
        if v is not None:
            same_bits(v, w, f"{what} {nm}")


@pytest.mark.parametrize("C,M,gdt,odt,with_y,with_gout,params", BN_BWD)
def test_bn_train_bwd(dev, C, M, gdt, odt, with_y, with_gout, params):
    """the backward alone: `saved` (mean, rstd) computed here in float64 and rounded to the fp32 the kernel reads"""
    from hulc2_amd import kernels as kn

    what = f"bn bwd C={C} M={M} dy={gdt} out={odt} y={with_y} g_out={with_gout} params={params}"
    g = _gen("bnb", C, M, str(gdt), str(odt), with_y, with_gout, params)
    z64, ga64, _, dy64, y64, mean64, rstd64 = _bn_bwd_inputs(g, C, M, gdt, with_y)
    mean64, rstd64 = rnd(mean64, F32), rnd(rstd64, F32)
    bg64, bb64 = (rnd(_randn(g, C) * M ** 0.5, F32), rnd(_randn(g, C) * M ** 0.5, F32)) if params == "accumulate" else (None, None)
    z, ga, dy = _in(dev, z64, F32), _in(dev, ga64, F32), _in(dev, dy64, gdt)
    y = _in(dev, y64, gdt) if with_y else None
    saved = _in(dev, torch.stack([mean64, rstd64]), F32)
    r64 = _bn_bwd_ref(dy64, y64, z64, ga64, mean64, rstd64, bg64, bb64, torch.float64)
    r32 = _bn_bwd_ref(dy64, y64, z64, ga64, mean64, rstd64, bg64, bb64, torch.float32)
    call = lambda: _bn_bwd_call(dev, kn, what, M, C, dy, y, z, ga, saved, odt, with_gout, params, bg64, bb64)
    _bn_bwd_check("nhwc_bn_train_bwd", what, call(), call(), r64, r32, gdt, odt)


@pytest.mark.parametrize("C,M,gdt", [(8, 1000, BF), (384, 257, F32), (2048, 3, BF), (64, 8192, BF)])
def test_bn_train_fwd_bwd_pair(dev, C, M, gdt):
    """forward and backward as the trunk chains them: the backward reads the forward's own y and (mean, rstd); the float64 reference knows
    neither and differentiates BatchNorm + ReLU from z (at M = 8192 with the channel means 16 standard deviations out)"""
    from hulc2_amd import kernels as kn

    what = f"bn pair C={C} M={M} {gdt}"
    g = _gen("bnp", C, M, str(gdt))
    z64, ga64, be64, dy64, _, mean64, rstd64 = _bn_bwd_inputs(g, C, M, gdt, False)
    if M == 8192:
        z64 = rnd(z64 + 16.0 * (z64.std(0) + 1.0), F32)
        mean64 = z64.mean(0)
        rstd64 = 1.0 / torch.sqrt(((z64 - mean64) ** 2).mean(0) + EPS)
    z, ga, be, dy = _in(dev, z64, F32), _in(dev, ga64, F32), _in(dev, be64, F32), _in(dev, dy64, gdt)
    y, sv = out_flat(dev, M * C, gdt), out_flat(dev, 2 * C, F32)
    kn.nhwc_bn_train_fwd(z, M, C, ga, be, EPS, 0.1, None, None, y.t.reshape(M, C), relu=True, saved=sv.t.reshape(2, C))
    torch.cuda.synchronize()
    y.assert_guards(f"{what} y")
    # the mask is the forward's own (a y within rounding of zero may fall on either side: the reference takes the side the forward took)
    y64 = y.value().reshape(M, C).double().cpu()
    r64 = _bn_bwd_ref(dy64, y64, z64, ga64, mean64, rstd64, None, None, torch.float64)
    m32 = z64.float().mean(0)
    r32 = _bn_bwd_ref(dy64, y64, z64, ga64, m32, 1.0 / torch.sqrt(((z64.float() - m32) ** 2).mean(0) + EPS), None, None, torch.float32)
    call = lambda: _bn_bwd_call(dev, kn, what, M, C, dy, y.t.reshape(M, C), z, ga, sv.t.reshape(2, C), gdt, True, "write", None, None)
    _bn_bwd_check("nhwc_bn_train fwd+bwd", what, call(), call(), r64, r32, gdt, gdt)


def test_bn_train_bwd_refusals(dev):
    from hulc2_amd import kernels as kn

    g = _gen("bn bwd refusals")

    def attempt(C, M, message, lead=0, rows=4):
        z, dy = _in(dev, _randn(g, rows, C), F32, lead=lead), _in(dev, _randn(g, rows, C), F32)
        ga, sv = _in(dev, _rand(g, C), F32), _in(dev, 0.5 + _rand(g, 2, C), F32)
        dz, dg, db = out_flat(dev, rows * C, F32), out_flat(dev, C, F32), out_flat(dev, C, F32)
        refused(lambda: kn.nhwc_bn_train_bwd(dy, None, z, M, C, ga, sv, dz.t.reshape(rows, C), dgamma=dg.t.reshape(C), dbeta=db.t.reshape(C)), message, dz, dg, db)

    shape = "hulc_nhwc_bn_train_bwd: C must be a multiple of 8 (a divisor of 256 below 256)"
    attempt(24, 4, shape)
    attempt(12, 4, shape)
    attempt(2056, 4, shape)
    attempt(64, 0, shape)
    attempt(64, 4, "hulc_nhwc_bn_train_bwd: 16-byte aligned rows", lead=1)


# ------------------------------------------------------------------------------------------------
# max pool, forward and backward (hulc_maxpool_nhwc, hulc_maxpool_nhwc_bwd)
# ------------------------------------------------------------------------------------------------
# k, stride, pad, H, W
POOL = [
    (3, 2, 1, 7, 9),           # the stem's pool on odd sides
    (3, 2, 1, 8, 8),           # even sides: the last window's last row and column are padding
    (3, 2, 1, 1, 1),           # one pixel, one window, eight of its nine positions padding
    (2, 2, 0, 5, 6),           # the last row falls in no window: its gradient is exactly zero
    (3, 1, 1, 4, 5),           # nine overlapping windows per pixel
    (3, 3, 0, 7, 7),           # disjoint windows, the last row and column in none
]


def _pool_ref(x64, dy64, k, s, pad):
    """nn.MaxPool2d's forward and its recorded indices (the first maximum in scan order), the gradient a float64 scatter-add of dy over them"""
    y64, idx = F.max_pool2d(x64, k, s, pad, return_indices=True)
    N, C, H, W = x64.shape
    dx64 = torch.zeros(N, C, H * W, dtype=x64.dtype).scatter_add_(2, idx.reshape(N, C, -1), dy64.reshape(N, C, -1)).reshape(N, C, H, W)
    return y64, dx64


def _pool_case(dev, k, s, pad, H, W, C, dtype, tied):
    from hulc2_amd import kernels as kn

    N = 2
    what = f"maxpool k={k} s={s} pad={pad} {H}x{W} C={C} {dtype} {'tied' if tied else 'random'}"
    g = _gen("pool", k, s, pad, H, W, C, str(dtype), tied)
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    if tied:
        u = _rand(g, N, C, H, W)                                                 # {0, 1, 2, 3}: half exact zeros, the largest value the commonest
        x64 = torch.where(u < 0.5, 0.0, torch.where(u < 0.85, 3.0, torch.where(u < 0.95, 2.0, 1.0))).double()
        dy64 = _ints(g, N, C, OH, OW, lo=-8, hi=8) / 8                           # up to nine windows per pixel: |sum| <= 9, exact in bf16
    else:
        x64, dy64 = rnd(_randn(g, N, C, H, W), dtype), rnd(_randn(g, N, C, OH, OW), dtype)
        assert x64.unique().numel() == x64.numel(), "the random case is meant to have no ties"
    y64, dx64 = _pool_ref(x64, dy64, k, s, pad)
    x, dy = _in(dev, _nhwc(x64), dtype), _in(dev, _nhwc(dy64), dtype)

    def call():
        y, dx = out_flat(dev, N * OH * OW * C, dtype), out_flat(dev, N * H * W * C, dtype)
        kn.maxpool_nhwc(x, y.t.reshape(N, OH, OW, C), N, H, W, C, k, s, pad)
        kn.maxpool_nhwc_bwd(x, dy, dx.t.reshape(N, H, W, C), N, H, W, C, k, s, pad)
        torch.cuda.synchronize()
        y.assert_guards(f"{what} y")
        dx.assert_guards(f"{what} dx")
        return y.value().reshape(N, OH, OW, C), dx.value().reshape(N, H, W, C)

    y, dx = call()
    _equal(y, _nhwc(y64), dtype, f"{what} forward")
    if tied:
        _equal(dx, _nhwc(dx64), dtype, f"{what} backward")
    else:
        r32 = _pool_ref(x64.float(), dy64.float(), k, s, pad)[1]
        compare("maxpool_nhwc_bwd", "dx", dx, _nhwc(dx64), _nhwc(r32), MARGIN["SUM"], grad=True, out_dtype=dtype)
    K.RATIOS.setdefault("maxpool_nhwc_bwd", 0.0)
    y2, dx2 = call()
    same_bits(y, y2, f"{what} y")
    same_bits(dx, dx2, f"{what} dx")
    return x64, dx64


@pytest.mark.parametrize("dtype", (F32, BF), ids=("f32", "bf16"))
@pytest.mark.parametrize("C", (8, 64))
@pytest.mark.parametrize("k,s,pad,H,W", POOL)
def test_maxpool_tied(dev, k, s, pad, H, W, C, dtype):
    x64, dx64 = _pool_case(dev, k, s, pad, H, W, C, dtype, True)
    if H * W > 1:                                        # the case is about ties: a large share of the windows has more than one maximum
        win = F.unfold(F.pad(x64, (pad,) * 4, value=-1.0), k, stride=s).reshape(x64.shape[0], x64.shape[1], k * k, -1)
        tied = ((win == win.max(2, keepdim=True).values).sum(2) > 1).double().mean().item()
        assert tied > 0.4, f"only {tied:.0%} of the windows have a tie"
    if (k, s, pad) == (2, 2, 0):
        assert not dx64[:, :, 4, :].any(), "the uncovered last row takes no gradient in the reference either"


@pytest.mark.parametrize("k,s,pad,H,W", [(3, 2, 1, 7, 9), (3, 1, 1, 4, 5)])
def test_maxpool_random(dev, k, s, pad, H, W):
    _pool_case(dev, k, s, pad, H, W, 8, F32, False)


def test_maxpool_refusals(dev):
    from hulc2_amd import kernels as kn

    g = _gen("pool refusals")
    for C, k, pad, H in ((12, 3, 1, 4), (8, 3, 2, 4), (8, 3, 0, 2)):                 # C % 8; 2 * pad > k; the map smaller than a window
        x, dy = _in(dev, _randn(g, 1, H, H, C), F32), _in(dev, _randn(g, 1, H, H, C), F32)
        y, dx = out_flat(dev, H * H * C, F32), out_flat(dev, H * H * C, F32)
        refused(lambda: kn.maxpool_nhwc(x, y.t.reshape(1, H, H, C), 1, H, H, C, k, 2, pad), "hulc_maxpool_nhwc: bad geometry", y)
        refused(lambda: kn.maxpool_nhwc_bwd(x, dy, dx.t.reshape(1, H, H, C), 1, H, H, C, k, 2, pad), "hulc_maxpool_nhwc_bwd: bad geometry", dx)


# ------------------------------------------------------------------------------------------------
# zero-inserting / zero-padding scatter (hulc_nhwc_scatter)
# ------------------------------------------------------------------------------------------------
# H, W, C, Hy, Wy, step, off
SCATTER = [
    (5, 7, 8, 10, 14, 2, 0),       # the zero-inserted gradient of a stride-2 convolution, even destination
    (5, 7, 64, 9, 13, 2, 0),       # odd destination: the last placed row and column are the destination's last
    (4, 3, 16, 10, 9, 1, 3),       # zero padding by 3
    (3, 4, 8, 11, 12, 2, 1),       # a destination larger than needed: trailing rows and columns are zero
    (1, 1, 8, 1, 1, 1, 0),         # a copy of one pixel
]


@pytest.mark.parametrize("dtype", (F32, BF), ids=("f32", "bf16"))
@pytest.mark.parametrize("H,W,C,Hy,Wy,step,off", SCATTER)
def test_nhwc_scatter(dev, H, W, C, Hy, Wy, step, off, dtype):
    from hulc2_amd import kernels as kn

    N = 2
    what = f"scatter {H}x{W}x{C} -> {Hy}x{Wy} step {step} off {off} {dtype}"
    g = _gen("scatter", H, W, C, Hy, Wy, step, off, str(dtype))
    x64 = rnd(_randn(g, N, H, W, C), dtype)
    x64[0, 0, 0, 0] = 0.0
    ref = torch.zeros(N, Hy, Wy, C, dtype=torch.float64)
    ref[:, off:off + step * (H - 1) + 1:step, off:off + step * (W - 1) + 1:step] = x64
    x = _in(dev, x64, dtype)

    def call():
        y = out_flat(dev, N * Hy * Wy * C, dtype)            # sentinel-filled: every element must be written, the zeros included
        kn.nhwc_scatter(x, y.t.reshape(N, Hy, Wy, C), step, off)
        torch.cuda.synchronize()
        y.assert_guards(what)
        return y.value().reshape(N, Hy, Wy, C)

    y = call()
    _equal(y, ref, dtype, what)
    same_bits(y, call(), what)
    K.RATIOS.setdefault("nhwc_scatter", 0.0)


def test_nhwc_scatter_refusals(dev):
    from hulc2_amd import kernels as kn

    g = _gen("scatter refusals")
    message = "hulc_nhwc_scatter: the placed map must fit the destination (C a multiple of 8)"
    for H, W, C, Hy, Wy, step, off in ((5, 7, 8, 8, 14, 2, 0), (5, 7, 8, 10, 12, 2, 0), (4, 3, 8, 9, 9, 1, 6), (4, 3, 12, 10, 9, 1, 3)):
        x = _in(dev, _randn(g, 1, H, W, C), F32)
        y = out_flat(dev, Hy * Wy * C, F32)
        refused(lambda: kn.nhwc_scatter(x, y.t.reshape(1, Hy, Wy, C), step, off), message, y)


# ------------------------------------------------------------------------------------------------
# input normalisation (hulc_r3m_normalize, hulc_r3m_normalize_packed)
# ------------------------------------------------------------------------------------------------
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
OTHER = ((0.31, 0.62, 0.07), (0.5, 0.125, 0.33))
NORM_HW = [(H, W) for H in (1, 5) for W in (1, 2, 7, 8, 131, 200)]


def _frames(g, N, H, W):
    x = rnd(255.0 * _rand(g, N, 3, H, W), F32)
    x[:, :, 0, 0] = torch.tensor([0.0, 255.0, 0.0]).double()         # the exact ends of the range, in the first and the last pixel
    x[:, :, H - 1, W - 1] = torch.tensor([255.0, 0.0, 255.0]).double()
    return x


def _norm_ref(x, stats, dt):
    """((x / 255) - mean) / std as the kernel evaluates it: the host hands it mean and 1 / std as float32"""
    mean, std = (torch.tensor(s, dtype=torch.float32) for s in stats)
    inv = (1.0 / std) if dt == torch.float32 else 1.0 / std.double()
    return (x.to(dt) / 255.0 - mean.to(dt)[None, :, None, None]) * inv.to(dt)[None, :, None, None]


@pytest.mark.parametrize("H,W", NORM_HW)
def test_r3m_normalize_packed(dev, H, W):
    from hulc2_amd import kernels as kn

    N = 2
    stats = OTHER if (H, W) == (5, 7) else IMAGENET
    what = f"normalize_packed {H}x{W}"
    Wp = 2 * ((W - 1) // 2) + 8
    assert kn.r3m_packed_width(W) == Wp, f"packed width of W = {W}: {kn.r3m_packed_width(W)}, the stem reads columns 0..{Wp - 1}"
    g = _gen("normp", H, W)
    x64 = _frames(g, N, H, W)
    x = _in(dev, x64, F32)
    full64, full32 = torch.zeros(N, H + 6, Wp, 4, dtype=torch.float64), torch.zeros(N, H + 6, Wp, 4, dtype=torch.float64)
    full64[:, 3:3 + H, 3:3 + W, :3] = _nhwc(_norm_ref(x64, stats, torch.float64))
    full32[:, 3:3 + H, 3:3 + W, :3] = _nhwc(_norm_ref(x64, stats, torch.float32)).double()
    inside = torch.zeros(N, H + 6, Wp, 4, dtype=torch.bool)
    inside[:, 3:3 + H, 3:3 + W, :3] = True

    def call():
        xp = out_flat(dev, N * (H + 6) * Wp * 4, BF)         # sentinel-prefilled: the border and channel 3 must be WRITTEN as zeros
        kn.r3m_normalize_packed(x, xp.t.reshape(N, H + 6, Wp, 4), *stats)
        torch.cuda.synchronize()
        xp.assert_guards(what)
        return xp.value().reshape(N, H + 6, Wp, 4)

    got = call()
    border = got.cpu()[~inside]
    assert torch.equal(border, torch.zeros_like(border)), f"{what}: {int((border != 0).sum())} border / channel-3 elements are not zero"
    compare("r3m_normalize_packed", "interior", got.cpu()[inside], full64[inside], full32[inside], MARGIN["SUM"], out_dtype=BF)
    same_bits(got, call(), what)


@pytest.mark.parametrize("dtype", (BF, F32), ids=("bf16", "f32"))
@pytest.mark.parametrize("H,W", NORM_HW)
def test_r3m_normalize(dev, H, W, dtype):
    from hulc2_amd import kernels as kn

    N = 2
    stats = OTHER if (H, W) == (5, 7) else IMAGENET
    what = f"normalize {H}x{W} {dtype}"
    g = _gen("norm", H, W)
    x64 = _frames(g, N, H, W)
    x = _in(dev, x64, F32)

    def call():
        y = out_flat(dev, N * H * W * 8, dtype)
        kn.r3m_normalize(x, y.t.reshape(N, H, W, 8), *stats)
        torch.cuda.synchronize()
        y.assert_guards(what)
        return y.value().reshape(N, H, W, 8)

    got = call()
    pad = got.cpu()[..., 3:]
    assert torch.equal(pad, torch.zeros_like(pad)), f"{what}: channels 3..7 are not zero"
    compare("r3m_normalize", str(dtype)[6:], got[..., :3], _nhwc(_norm_ref(x64, stats, torch.float64)), _nhwc(_norm_ref(x64, stats, torch.float32)),
            MARGIN["SUM"], out_dtype=dtype)
    same_bits(got, call(), what)


# ------------------------------------------------------------------------------------------------
# the packed stem (hulc_r3m_stem_fwd): 7 x 7, stride 2, padding 3 on [N][H + 6][Wp][4] "double pixels"
# ------------------------------------------------------------------------------------------------
def _pack_input(x64):
    """(N, 3, H, W) -> the packed layout built directly (not through the normaliser): pixel (y, x) at [y + 3][x + 3] = (R, G, B, 0), zero border"""
    N, _, H, W = x64.shape
    xp = torch.zeros(N, H + 6, 2 * ((W - 1) // 2) + 8, 4, dtype=torch.float64)
    xp[:, 3:3 + H, 3:3 + W, :3] = _nhwc(x64)
    return xp


def _pack_weights(w64):
    """(Cout, 3, 7, 7) -> [Cout][7][8][4] with zeros at kw = 7 and c = 3, as the trunk packs its folded stem"""
    Cout = w64.shape[0]
    wp = torch.zeros(Cout, 7, 8, 4, dtype=torch.float64)
    wp[:, :, :7, :3] = w64.permute(0, 2, 3, 1)
    return wp.reshape(Cout, 224)


def _stem_case(dev, N, H, W, Cout, ydt, relu, lattice=True, bias=True):
    from hulc2_amd import kernels as kn

    what = f"stem N={N} {H}x{W} Cout={Cout} y={ydt} relu={relu} {'lattice' if lattice else 'random'}"
    g = _gen("stem", N, H, W, Cout, str(ydt), relu, lattice)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if lattice:       # every output is an integer of magnitude <= 147 + 4: exact in fp32 in any order, and exact in bf16
        x64, w64, b64 = _ints(g, N, 3, H, W, lo=-1, hi=1), _ints(g, Cout, 3, 7, 7, lo=-1, hi=1), _ints(g, Cout, lo=-4, hi=4)
    else:
        x64, w64, b64 = rnd(_randn(g, N, 3, H, W), BF), rnd(_randn(g, Cout, 3, 7, 7) / 147 ** 0.5, BF), rnd(0.1 * _randn(g, Cout), F32)
    xp, w, b = _in(dev, _pack_input(x64), BF), _in(dev, _pack_weights(w64), BF), (_in(dev, b64, F32) if bias else None)

    def ref(dt):
        z = F.conv2d(x64.to(dt), w64.to(dt), b64.to(dt) if bias else None, stride=2, padding=3)
        return _nhwc(torch.relu(z) if relu else z)

    def call():
        y = out_flat(dev, N * OH * OW * Cout, ydt)
        kn.r3m_stem_fwd(xp, w, b, y.t.reshape(N, OH, OW, Cout), N, H, W, Cout, relu=relu)
        torch.cuda.synchronize()
        y.assert_guards(what)
        return y.value().reshape(N, OH, OW, Cout)

    y, r64 = call(), ref(torch.float64)
    assert tuple(r64.shape) == (N, OH, OW, Cout)
    if lattice:
        _equal(y, r64, ydt, what)                        # (a read outside [N][H + 6][Wp][4] meets a NaN sentinel and fails here)
        K.RATIOS.setdefault("r3m_stem_fwd", 0.0)
    else:
        compare("r3m_stem_fwd", "y", y, r64, ref(torch.float32), MARGIN["SUM"], out_dtype=ydt)
    same_bits(y, call(), what)


# N, H, W, Cout, y type, relu
STEM = [
    (1, 1, 1, 64, BF, True),           # one output pixel: 127 rows of the 128-pixel tile are clamped duplicates
    (2, 2, 3, 64, F32, False),
    (2, 9, 10, 64, BF, False),         # even W, OW = 5
    (2, 10, 9, 128, BF, True),         # odd W, OW = 5 from the other packed width; the 128-channel tile
    (2, 37, 50, 64, F32, True),        # 950 pixels: seven full tiles and a ragged one
    (2, 37, 50, 128, BF, False),
    (127, 1, 1, 64, BF, True),         # one pixel short of a tile
    (128, 1, 2, 128, F32, True),       # exactly one tile
    (129, 2, 1, 64, F32, False),       # one pixel into the second tile
    (43, 2, 5, 128, BF, True),         # 129 pixels over 43 images of 1 x 3
]


@pytest.mark.parametrize("N,H,W,Cout,ydt,relu", STEM)
def test_r3m_stem_lattice(dev, N, H, W, Cout, ydt, relu):
    _stem_case(dev, N, H, W, Cout, ydt, relu)


def test_r3m_stem_tall_tiles(dev):
    """Cout = 64 from 131,072 pixels on: 256-pixel tiles, four waves stacked over the pixels — the instance a real batch of frames runs"""
    _stem_case(dev, 277, 37, 50, 64, BF, True)           # 277 * 19 * 25 = 131,575 pixels, ragged in the last tile


def test_r3m_stem_no_bias(dev):
    _stem_case(dev, 2, 9, 10, 64, F32, True, bias=False)


@pytest.mark.parametrize("Cout,ydt", [(64, F32), (128, BF)])
def test_r3m_stem_random(dev, Cout, ydt):
    _stem_case(dev, 2, 37, 50, Cout, ydt, True, lattice=False)


def test_r3m_stem_refusals(dev):
    from hulc2_amd import kernels as kn

    g = _gen("stem refusals")
    x64 = _ints(g, 1, 3, 4, 4, lo=-1, hi=1)
    xp, w, b = _in(dev, _pack_input(x64), BF), _in(dev, torch.zeros(32, 224, dtype=torch.float64), BF), _in(dev, torch.zeros(32, dtype=torch.float64), F32)
    y = out_flat(dev, 2 * 2 * 32, BF)
    refused(lambda: kn.r3m_stem_fwd(xp, w, b, y.t.reshape(1, 2, 2, 32), 1, 4, 4, 32), "hulc_r3m_stem_fwd: bad geometry (Cout must be a multiple of 64)", y)
    refused(lambda: kn.r3m_stem_fwd(xp, w, b, y.t.reshape(1, 2, 2, 32), 0, 4, 4, 64), "hulc_r3m_stem_fwd: bad geometry (Cout must be a multiple of 64)", y)
