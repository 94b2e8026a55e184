"""Kernel-level tests of csrc/ffn_fused.hip: kn.ffn_fwd / kn.ffn_bwd called directly, against the float64 references of tests/seqref.py.

  * exact cases: integer lattices (seqref.ffn_lattice) for which every fp32 sum is exact in any order and every bf16 rounding point rounds an
    exactly known value, so all outputs must equal the float64 emulation BIT FOR BIT: forward and backward, the hidden-slice partials left
    in the workspace (f = None / dx = None, b2 in slice 0 only), dx_accumulate and accumulate_params, dropout 0 and 0.5 with the device
    RNG word set, token counts that make the 16 token groups walk 1 and 2 tiles unevenly, FF = 128 / 384 / 2048;
  * random cases at the model's magnitudes against the plain float64 reference, per row (kcheck.compare_rows), the yardstick being the CPU
    emulation of the kernel's bf16 rounding points with float32 accumulation; the pre-activation sits on a dyadic grid so that no ReLU
    gate can differ between the kernel and the reference;
  * refusals.
The pattern of a case (guard bands, replay, refusals) is that of tests/kcheck.py."""
import time

import pytest
import torch

from tests import kcheck as K
from tests import seqref as Q
from tests.kcheck import Guarded, compare_rows, out_flat, refused, same_bits

pytestmark = pytest.mark.gpu

# margin * max(e_ref, 2^-23) per tensor, e_ref = the CPU rounding-point emulation with float32 accumulation against float64, per row.  The
# kernel and the emulation realise the same rounding points and differ in fp32 summation order only (a float64-accumulating emulation scores
# 1.00 x e_ref in every case: tests/test_seqref_cpu.py), so every tensor gets 2.
MARGIN = {"f": 2.0, "dx": 2.0, "dW1": 2.0, "db1": 2.0, "dW2": 2.0, "f_slab": 2.0, "dx_slab": 2.0}

BF16, F32 = torch.bfloat16, torch.float32
REFUSED_FWD = "hulc_ffn_fwd: needs d_model 128 and dim_feedforward a multiple of 128"
REFUSED_BWD = "hulc_ffn_bwd: needs d_model 128 and dim_feedforward a multiple of 128"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    K.report("tests/test_ffn_kernel_gpu.py")
    print(f"[kcheck-time] tests/test_ffn_kernel_gpu.py {time.time() - t0:.1f} s")


def _reference(build, *args):
    """the CPU references on at most 8 threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(8, n))
    try:
        return build(*args)
    finally:
        torch.set_num_threads(n)


class _Operands:
    def __init__(self, dev, ops, p):
        from hulc2_amd import kernels as kn

        kn.set_compute("bf16")
        self.T, self.FF, self.p = ops["x"].shape[0], ops["W1"].shape[0], p
        self.x, self.df = ops["x"].to(dev, F32), ops["df"].to(dev, F32)
        self.W1, self.W2 = ops["W1"].to(dev, BF16), ops["W2"].to(dev, BF16)
        self.W1T, self.W2T = self.W1.t().contiguous(), self.W2.t().contiguous()
        self.b1, self.b2 = ops["b1"].to(dev, F32), ops["b2"].to(dev, F32)
        for name in ("x", "df", "W1", "W2", "b1", "b2"):              # the references were given exactly what the kernel reads
            assert torch.equal(getattr(self, name).double().cpu(), ops[name]), f"{name} is not exact in its storage type"
        if p > 0.0:
            kn.reset_step_state(dev, seed=Q.RNG_WORD)
            assert int(kn.step_state(dev)[0].item()) == Q.RNG_WORD

    def fwd(self, f):
        from hulc2_amd import kernels as kn

        ws = kn.ffn_fwd(self.x, self.W1, self.b1, self.W2, self.b2, self.T, 128, self.FF, self.p, Q.FFN_SEED, None if f is None else f.t)
        torch.cuda.synchronize()
        return ws[:self.FF // 128 * self.T * 128].view(self.FF // 128, self.T, 128)

    def bwd(self, dx, dW1, db1, dW2, accumulate_params=False, dx_accumulate=False):
        from hulc2_amd import kernels as kn

        ws = kn.ffn_bwd(self.x, self.df, self.W1, self.b1, self.W1T, self.W2T, self.T, 128, self.FF, self.p, Q.FFN_SEED,
                        None if dx is None else dx.t, dW1.t, db1.t, dW2.t, accumulate_params=accumulate_params, dx_accumulate=dx_accumulate)
        torch.cuda.synchronize()
        return ws[:self.FF // 128 * self.T * 128].view(self.FF // 128, self.T, 128)

    def grads(self, dev, init=None):
        """guarded dW1, db1, dW2 (sentinel-filled, or holding init[name])"""
        i = init or {}
        return (Guarded(dev, self.FF, 128, init=i.get("dW1")), out_flat(dev, self.FF, init=i.get("db1")), Guarded(dev, 128, self.FF, init=i.get("dW2")))


def _exact(got, want64, what):
    got, want = got.detach().cpu().reshape(-1), want64.float().reshape(-1)
    assert torch.equal(want.double(), want64.reshape(-1)), f"{what}: the expected values are not fp32 numbers (a broken lattice)"
    bad = got != want
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference; first at flat index {i}: "
                             f"kernel {got[i].item()!r}, reference {want[i].item()!r}")


def _slabs_exact(slab, want64, what):
    for s in range(want64.shape[0]):                                  # slice by slice: b2 rides in slice 0 only
        _exact(slab[s], want64[s], f"{what} slice {s}")


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("FF", Q.FFN_LATTICE_FF)
@pytest.mark.parametrize("T", Q.FFN_LATTICE_T)
def test_ffn_lattice_is_bit_exact(dev, T, FF, p):
    ops, want, st = _reference(Q.ffn_lattice_case, T, FF, p)
    o = _Operands(dev, ops, p)
    who = f"ffn lattice T {T} FF {FF} p {p}"
    # ---- forward: summed output, then the slice partials left in the workspace
    f = Guarded(dev, T, 128)
    slab = o.fwd(f)
    f.assert_guards(f"{who} f")
    _exact(f.value(), want["f"], f"{who} f")
    _slabs_exact(slab, want["f_slab"], f"{who} f partials behind a summed call")
    first = f.value()
    o.fwd(f)
    same_bits(first, f.value(), f"{who} f")
    _slabs_exact(o.fwd(None), want["f_slab"], f"{who} f partials (f = None)")
    # ---- backward: stored
    dx, (dW1, db1, dW2) = Guarded(dev, T, 128), o.grads(dev)
    o.bwd(dx, dW1, db1, dW2)
    outs = dict(dx=dx, dW1=dW1, db1=db1, dW2=dW2)
    for name, g in outs.items():
        g.assert_guards(f"{who} {name}")
        _exact(g.value(), want[name], f"{who} {name}")
    first = {name: g.value() for name, g in outs.items()}
    o.bwd(dx, dW1, db1, dW2)
    for name, g in outs.items():
        same_bits(first[name], g.value(), f"{who} {name}")
    # ---- backward: dx = None leaves the slice partials; parameters accumulate onto integer contents
    gen = torch.Generator().manual_seed(T + FF)
    init = {n: torch.randint(-5, 6, tuple(want[n].shape), generator=gen).double() for n in ("dx", "dW1", "db1", "dW2")}
    dW1, db1, dW2 = o.grads(dev, init)
    slab = o.bwd(None, dW1, db1, dW2, accumulate_params=True)
    _slabs_exact(slab, want["dx_slab"], f"{who} dx partials (dx = None)")
    for name, g in (("dW1", dW1), ("db1", db1), ("dW2", dW2)):
        g.assert_guards(f"{who} {name} accumulated")
        _exact(g.value(), want[name] + init[name], f"{who} {name} accumulated")
    # ---- backward: dx accumulates, parameters are stored over what was there
    dx = Guarded(dev, T, 128, init=init["dx"])
    o.bwd(dx, dW1, db1, dW2, dx_accumulate=True)
    dx.assert_guards(f"{who} dx accumulated")
    _exact(dx.value(), want["dx"] + init["dx"], f"{who} dx accumulated")
    for name, g in (("dW1", dW1), ("db1", db1), ("dW2", dW2)):
        _exact(g.value(), want[name], f"{who} {name} stored over old contents")


@pytest.mark.parametrize("T,FF,p", Q.FFN_RANDOM_CASES)
def test_ffn_random_against_float64(dev, T, FF, p):
    ops, plain, e32, _ = _reference(Q.ffn_random_case, T, FF, p)
    o = _Operands(dev, ops, p)
    who = f"T{T} FF{FF} p{p}"
    f, dx, (dW1, db1, dW2) = Guarded(dev, T, 128), Guarded(dev, T, 128), o.grads(dev)
    f_slab = o.fwd(f).clone()
    dx_slab = o.bwd(dx, dW1, db1, dW2).clone()
    got = dict(f=f.value(), dx=dx.value(), dW1=dW1.value(), db1=db1.value().reshape(-1), dW2=dW2.value(), f_slab=f_slab, dx_slab=dx_slab)
    for g in (f, dx, dW1, db1, dW2):
        g.assert_guards(who)
    for name, t in got.items():
        compare_rows("ffn_fwd" if name.startswith("f") else "ffn_bwd", f"{name} {who}", Q.ffn_rows(name, t), Q.ffn_rows(name, plain[name]),
                     Q.ffn_rows(name, e32[name]), MARGIN[name])
    first = {n: g.value() for n, g in (("f", f), ("dx", dx), ("dW1", dW1), ("db1", db1), ("dW2", dW2))}
    o.fwd(f)
    o.bwd(dx, dW1, db1, dW2)
    for n, g in (("f", f), ("dx", dx), ("dW1", dW1), ("db1", db1), ("dW2", dW2)):
        same_bits(first[n], g.value(), f"{who} {n}")


def test_ffn_refusals(dev):
    ops, _, _ = _reference(Q.ffn_lattice, 4, 128, 3)
    o = _Operands(dev, ops, 0.0)
    from hulc2_amd import kernels as kn

    f, dx, (dW1, db1, dW2) = Guarded(dev, 4, 128), Guarded(dev, 4, 128), o.grads(dev)

    def fwd(T, D, FF):
        return lambda: kn.ffn_fwd(o.x, o.W1, o.b1, o.W2, o.b2, T, D, FF, 0.0, Q.FFN_SEED, f.t)

    def bwd(T, D, FF):
        return lambda: kn.ffn_bwd(o.x, o.df, o.W1, o.b1, o.W1T, o.W2T, T, D, FF, 0.0, Q.FFN_SEED, dx.t, dW1.t, db1.t, dW2.t)

    for T, D, FF in ((4, 64, 128), (4, 256, 128), (4, 128, 64), (4, 128, 192), (4, 128, 0), (0, 128, 128), (-1, 128, 128)):
        refused(fwd(T, D, FF), REFUSED_FWD, f)
        refused(bwd(T, D, FF), REFUSED_BWD, dx, dW1, db1, dW2)
    refused(lambda: kn.ffn_bwd(o.x, o.df, o.W1, o.b1, o.W1T, o.W2T, 4, 128, 128, 0.0, Q.FFN_SEED, dx.t, None, db1.t, dW2.t),
            "hulc_ffn_bwd: null pointer", dx, db1, dW2)
