"""Kernel-level tests of csrc/mlp2_rows.hip: kn.mlp2_rows_fwd / kn.mlp2_rows_bwd called directly (plain, no dropout), against the float64
references of tests/mlpref.py.

  * exact cases: integer lattices (mlpref.mlp2_lattice) on which every fp32 sum is exact in any order and every bf16 rounding point rounds an
    exactly known value (hidden values above 256 included): y, h, dh and dx must equal the float64 reference BIT FOR BIT, plain and with
    split operands (W1_lo, W2_lo; inputs with a non-zero lo part);
  * random cases at the model's magnitudes, per row (kcheck.compare_rows), the yardstick being the CPU emulation of the same rounding points
    with float32 accumulation.  The pre-activation sits on a dyadic grid, so no ReLU gate and no rounding of the hidden tile can differ:
    h must still be bit-exact; dh (bf16) is compared with the float64 value before its rounding, half an ulp allowed (kcheck.half_ulp);
    dx is teacher-forced: the reference multiplies the dh the kernel stored;
  * dx = None leaves h and dh identical; guard bands on y, dx, h, dh; replay for bits; refusals.
T in {1, 31, 32, 33, 65, 96} x H in {128, 384} x OUT in {32, 64, 96, 128}: every OT instance, both exchange variants, the ragged last
32-row block.  The pattern of a case is that of tests/kcheck.py."""
import time

import pytest
import torch

from tests import kcheck as K
from tests import mlpref as R
from tests.kcheck import Guarded, compare_rows, half_ulp, refused, same_bits

pytestmark = pytest.mark.gpu

# margin * max(e_ref, 2^-23) per tensor, e_ref = the CPU emulation of the same rounding points with float32 accumulation against float64,
# per row: kernel and emulation differ in fp32 summation order only (tests/test_ffn_kernel_gpu.py: 2).  Largest ratios measured on an
# MI355X ([kcheck-max] lines of this file):
#   mlp2_rows_fwd 0.74   mlp2_rows_fwd x3 1.59   mlp2_rows_bwd dh 0.12   mlp2_rows_bwd dx 0.38
MARGIN = 2.0

BF16, F32 = torch.bfloat16, torch.float32
REFUSED_FWD = "hulc_mlp2_rows_fwd: needs K = 128, H a multiple of 128, OUT in {32, 64, 96, 128}, 16-byte aligned operands"
REFUSED_BWD = "hulc_mlp2_rows_bwd: needs K = 128, H a multiple of 128, OUT in {32, 64, 96, 128}, 16-byte aligned operands"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hulc2_amd import kernels as kn

    kn.set_compute("bf16")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    K.report("tests/test_mlp2_rows_kernel_gpu.py")
    print(f"[kcheck-time] tests/test_mlp2_rows_kernel_gpu.py {time.time() - t0:.1f} s")


def _reference(build, *args, **kw):
    """the CPU references on at most 8 threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(8, n))
    try:
        return build(*args, **kw)
    finally:
        torch.set_num_threads(n)


class _Operands:
    def __init__(self, dev, ops):
        self.dev = dev
        self.T, self.H, self.OUT = ops["x"].shape[0], ops["W1"].shape[0], ops["W2"].shape[0]
        types = dict(x=F32, dy=F32, b1=F32, b2=F32, W1=BF16, W2=BF16, W1_lo=BF16, W2_lo=BF16)
        for name, t in ops.items():
            setattr(self, name, t.to(dev, types[name]).contiguous())
            assert torch.equal(getattr(self, name).double().cpu(), t), f"{name} is not exact in its storage type"
        self.W1T, self.W2T = self.W1.t().contiguous(), self.W2.t().contiguous()
        self.x3 = "W1_lo" in ops

    def outputs(self):
        d = self.dev
        return dict(y=Guarded(d, self.T, self.OUT), dx=Guarded(d, self.T, 128), h=Guarded(d, self.T, self.H, BF16), dh=Guarded(d, self.T, self.H, BF16))

    def fwd(self, y, x3=None):
        from hulc2_amd import kernels as kn

        x3 = self.x3 if x3 is None else x3
        kn.mlp2_rows_fwd(self.x, self.W1, self.b1, self.W2, self.b2, y.t, self.W1_lo if x3 else None, self.W2_lo if x3 else None)
        torch.cuda.synchronize()

    def bwd(self, dx, h, dh):
        from hulc2_amd import kernels as kn

        kn.mlp2_rows_bwd(self.x, self.dy, self.W1, self.b1, self.W1T, self.W2T, None if dx is None else dx.t, h.t, dh.t)
        torch.cuda.synchronize()


def _exact(got, want64, what):
    got, want = got.detach().float().cpu().reshape(-1), want64.float().reshape(-1)
    assert torch.equal(want.double(), want64.reshape(-1)), f"{what}: the expected values are not fp32 numbers (a broken lattice)"
    bad = got != want
    if bad.any():
        i = int(bad.nonzero()[0])
        cols = want64.shape[-1]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference; first at row {i // cols}, "
                             f"column {i % cols}: kernel {got[i].item()!r}, reference {want[i].item()!r}")


def _run_all(o: _Operands, who):
    """forward and backward into guarded outputs, guards checked, replayed for bits, dx = None leaves h and dh as they were"""
    out = o.outputs()
    o.fwd(out["y"])
    o.bwd(out["dx"], out["h"], out["dh"])
    for name, g in out.items():
        g.assert_guards(f"{who} {name}")
    first = {name: g.value() for name, g in out.items()}
    o.fwd(out["y"])
    o.bwd(out["dx"], out["h"], out["dh"])
    for name, g in out.items():
        same_bits(first[name], g.value(), f"{who} {name}")
    h2, dh2 = Guarded(o.dev, o.T, o.H, BF16), Guarded(o.dev, o.T, o.H, BF16)
    o.bwd(None, h2, dh2)
    for name, g in (("h", h2), ("dh", dh2)):
        g.assert_guards(f"{who} {name} (dx = None)")
        assert torch.equal(g.value(), first[name]), f"{who}: {name} of the run without dx differs from the run with dx"
    return first


@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("OUT", R.MLP2_OUT)
@pytest.mark.parametrize("H", R.MLP2_H)
def test_mlp2_lattice_is_bit_exact(dev, H, OUT, x3):
    for T in R.MLP2_T:
        ops, want = _reference(R.mlp2_lattice, T, H, OUT, R.mlp2_seed(T, H, OUT, x3), x3)
        who = f"mlp2 lattice T {T} H {H} OUT {OUT} x3 {x3}"
        got = _run_all(_Operands(dev, ops), who)
        for name, w in zip(("y", "h", "dh", "dx"), want):
            _exact(got[name], w, f"{who} {name}")


def _minus_half_ulp(got, ref64, dtype):
    """`got` with half an ulp of the bf16 storage type forgiven per element: what compare_rows is handed for a bf16 output"""
    got, ref64 = got.detach().double().cpu(), ref64.double()
    d = got - ref64
    return ref64 + torch.sign(d) * (d.abs() - half_ulp(ref64, dtype)).clamp_min(0.0)


@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("OUT", R.MLP2_OUT)
@pytest.mark.parametrize("H", R.MLP2_H)
def test_mlp2_random_against_float64(dev, H, OUT, x3):
    for T in R.MLP2_T:
        ops, ref, e32 = _reference(R.mlp2_random, T, H, OUT, R.mlp2_seed(T, H, OUT, x3), x3)
        who = f"T{T} H{H} O{OUT}"
        o = _Operands(dev, ops)
        got = _run_all(o, who)
        compare_rows("mlp2_rows_fwd x3" if x3 else "mlp2_rows_fwd", f"y {who}", got["y"], ref[0], e32[0], MARGIN)
        if x3:
            continue                                                  # (the backward has no split-operand variant: checked by the plain case)
        _exact(got["h"], ref[1], f"{who} h (the dyadic pre-activation is exact)")
        compare_rows("mlp2_rows_bwd dh", f"dh {who}", _minus_half_ulp(got["dh"], ref[5], BF16), ref[5], e32[5], MARGIN)       # (e32[5]: before rounding)
        lo = {k: ops[k] for k in ("W1_lo", "W2_lo") if k in ops}
        args = {k: ops[k] for k in ("x", "W1", "b1", "W2", "b2", "dy")}
        fed = got["dh"].double().cpu()
        dx64 = _reference(R.mlp2_ref, **args, **lo, dh_fed=fed)[3]
        dx32 = _reference(R.mlp2_ref, **args, **lo, dh_fed=fed, acc=torch.float32)[3]
        compare_rows("mlp2_rows_bwd dx", f"dx {who}", got["dx"], dx64, dx32, MARGIN)


def test_mlp2_refusals(dev):
    from hulc2_amd import kernels as kn

    ops, _ = _reference(R.mlp2_lattice, 4, 128, 32, 1, True)
    o = _Operands(dev, ops)
    out = o.outputs()
    y, dx, h, dh = out["y"], out["dx"], out["h"], out["dh"]
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=dev)

    def fwd(W1, W2, b1, b2, K_=128, y_=y, lo=(None, None)):
        return lambda: kn._call("hulc_mlp2_rows_fwd", o.x, W1, b1, W2, b2, lo[0], lo[1], 4, K_, W1.shape[0], W2.shape[0], y_.t)

    def bwd(W1, W2T, b1, K_=128, dy=o.dy, dx_=dx, h_=h, dh_=dh):
        return lambda: kn._call("hulc_mlp2_rows_bwd", o.x, dy, W1, b1, o.W1T, W2T, 4, K_, W1.shape[0], W2T.shape[1], dx_.t, h_.t, dh_.t)

    refused(fwd(o.W1, o.W2, o.b1, o.b2, K_=64), REFUSED_FWD, y)
    refused(bwd(o.W1, o.W2T, o.b1, K_=64), REFUSED_BWD, dx, h, dh)
    refused(fwd(z(192, 128), z(32, 192), z(192, dt=F32), o.b2), REFUSED_FWD, y)                       # H = 192
    refused(bwd(z(192, 128), z(192, 32), z(192, dt=F32)), REFUSED_BWD, dx, h, dh)
    for OUT in (160, 16):
        refused(fwd(o.W1, z(OUT, 128), o.b1, z(OUT, dt=F32)), REFUSED_FWD, y)
        refused(bwd(o.W1, z(128, OUT), o.b1), REFUSED_BWD, dx, h, dh)
    y1 = Guarded(dev, 4, 32, lead=1)
    refused(fwd(o.W1, o.W2, o.b1, o.b2, y_=y1), "hulc_mlp2_rows_fwd: null or misaligned pointer", y1)
    dy1 = torch.zeros(4 * 32 + 4, device=dev)[1:129].view(4, 32)
    refused(bwd(o.W1, o.W2T, o.b1, dy=dy1), "hulc_mlp2_rows_bwd: null or misaligned pointer", dx, h, dh)
    h1 = Guarded(dev, 4, 128, BF16, lead=1)
    refused(bwd(o.W1, o.W2T, o.b1, h_=h1), "hulc_mlp2_rows_bwd: null or misaligned pointer", dx, h1, dh)
    refused(bwd(o.W1, o.W2T, o.b1, dh_=h1), "hulc_mlp2_rows_bwd: null or misaligned pointer", dx, h, h1)
    refused(fwd(o.W1, o.W2, o.b1, o.b2, lo=(o.W1_lo, None)), "hulc_mlp2_rows_fwd: both remainder arrays or none", y)
    refused(fwd(o.W1, o.W2, o.b1, o.b2, lo=(None, o.W2_lo)), "hulc_mlp2_rows_fwd: both remainder arrays or none", y)
