"""Kernel-level tests of csrc/rnn_wavefront.hip: kn.rnn_wavefront called directly, against seqref.rnn_sweep, the recurrence exactly as
include/hulc2_amd.h states it (tests/test_seqref_cpu.py checks that reference against torch's nn.RNN and its autograd backward).

  * exact cases: integer lattices (seqref.rnn_lattice: sparse +-1 weights, integer add terms) for which every fp32 sum is exact in any order
    and the bf16 rounding of the state, once per wave step, rounds an exactly known value: all state rows and both bf16 mirrors must equal
    the float64 emulation BIT FOR BIT.  Forward mode = relu, add1 + add1c + four biases, z_step > 0, row-major weights; backward mode =
    mask1 / mask2 with pitch 2H and negative steps, z_step < 0, transposed weights.  Weights, add1 and add1c are views with a pitch of
    their own inside NaN-filled allocations; the state buffer is sentinel-filled, with a gap of one state row after the B rows of every
    wave step (where a batch row B would land), and zero_edges must clear exactly row 0 and the first half of row S+1;
  * random cases at the model's magnitudes against the plain float64 reference, per (wave step, batch row, half);
  * refusals, among them mixed weight layouts with zero_edges: a refused call must not have launched its clearing kernels.
Every launch is followed by kn.check_faults (the kernel's device-wide barrier reports a timeout there)."""
import time

import pytest
import torch

from tests import kcheck as K
from tests import seqref as Q
from tests.kcheck import Guarded, compare_rows, refused, same_bits

pytestmark = pytest.mark.gpu

# margin * max(e_ref, 2^-23), e_ref = the CPU emulation (state rounded to bf16 once per wave step, float32 accumulation) against float64,
# per (wave step, batch row, half).  Kernel and emulation differ in fp32 summation order only.
MARGIN = {"forward": 2.0, "backward": 2.0}

H = 2048
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    K.report("tests/test_rnn_kernel_gpu.py")
    print(f"[kcheck-time] tests/test_rnn_kernel_gpu.py {time.time() - t0:.1f} s")


def _reference(build, *args):
    """the CPU references on at most 8 threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(8, n))
    try:
        return build(*args)
    finally:
        torch.set_num_threads(n)


def _padded(dev, t64, pad, dtype=F32):
    """t64 (..., n) as a view of pitch n + pad inside a NaN-filled allocation: a read outside the view poisons the result"""
    buf = torch.full((*t64.shape[:-1], t64.shape[-1] + pad), float("nan"), dtype=dtype, device=dev)
    view = buf[..., :t64.shape[-1]]
    view.copy_(t64)
    assert torch.equal(view.double().cpu(), t64), "an operand is not exact in its storage type"
    return view


class _Sweep:
    """one direction's operands on the device, laid out as the decoder lays them out"""

    def __init__(self, dev, S, B, ops, backward, wpad=64, sentinel=True):
        from hulc2_amd import kernels as kn

        kn.set_compute("bf16")
        self.dev, self.S, self.B, self.backward = dev, S, B, backward
        # weights: element (n, k) at w[n * ld + k], or w[k * ld + n] for the transposed layout of the backward sweep; ld = H + wpad
        self.w = [_padded(dev, ops[n].t().contiguous() if backward else ops[n], wpad, BF16) for n in ("wA", "wB1", "wB2")]
        self.ld_z = B * 2 * H + 2 * H                                  # one state row of gap after every wave step's B rows
        self.z = Guarded(dev, S + 2, B * 2 * H, ld=self.ld_z, init=None if sentinel else torch.zeros(S + 2, B * 2 * H))
        kw = dict(relu=bool(ops.get("relu")), mirror_t=B % 8 == 0, zero_edges=sentinel)
        add1 = ops["add1"]                                             # (S, B, H) by wave step
        if backward:                                                   # walked from the far end with negative steps, like the state
            self.add1 = _padded(dev, add1.flip(0), 8)
            kw.update(add1=self.add1[S - 1], add1_step=-self.add1.stride(0), ld_add1=self.add1.stride(1))
            # masks: the forward pass's stored activations, (S + 2, B, 2H) rows of pitch 2H; mask1[tau] in the second half of row S - tau,
            # mask2[tau] in the first half of row S + 1 - tau; everything else NaN (never kept)
            m = torch.full((S + 2, B, 2 * H), float("nan"), dtype=torch.float64)
            for tau in range(S):
                m[S - tau, :, H:] = ops["mask1"][tau]
            for tau in range(1, S + 1):
                m[S + 1 - tau, :, :H] = ops["mask2"][tau]
            self.m = m.to(dev, F32)
            kw.update(mask1=self.m[S, :, H:], mask1_step=-B * 2 * H, ld_mask1=2 * H, mask2=self.m[S + 1, :, :H], mask2_step=-B * 2 * H, ld_mask2=2 * H)
            self.z0, self.z_step = self.z.t[S + 1], -self.ld_z
        else:
            self.add1 = _padded(dev, add1, 8)
            kw.update(add1=self.add1[0], add1_step=self.add1.stride(0), ld_add1=self.add1.stride(1))
            self.z0, self.z_step = self.z.t[0], self.ld_z
        if ops.get("add1c") is not None:
            self.add1c = _padded(dev, ops["add1c"], 16)
            kw.update(add1c=self.add1c)
        for name in ("bias1", "bias2"):
            if name in ops:
                setattr(self, name, tuple(None if b is None else b.to(dev, F32) for b in ops[name]))
                kw[name] = getattr(self, name)
        self.kw = kw

    def run(self, transposed=None, **override):
        from hulc2_amd import kernels as kn

        a = dict(S=self.S, B=self.B, H=H)
        a.update({k: override.pop(k) for k in ("S", "B", "H") if k in override})
        w = override.pop("w", self.w)
        z16, z16t = kn.rnn_wavefront(self.z0, self.z_step, a["S"], a["B"], a["H"], w[0], w[1], w[2], self.backward if transposed is None else transposed,
                                     **{**self.kw, **override})
        torch.cuda.synchronize()
        kn.check_faults(self.dev)
        return z16, z16t

    def rows(self):
        """the fp32 state rows in SWEEP order (S + 2, B, 2H)"""
        z = self.z.value().view(self.S + 2, self.B, 2 * H)
        return z.flip(0) if self.backward else z

    def mirrors(self, z16, z16t):
        """both bf16 mirrors in sweep order, the transposed one brought to (S + 2, B, 2H)"""
        S, B = self.S, self.B
        out = [z16.clone()]
        if z16t is not None:
            out.append(z16t.view(2 * H, S + 2, B).permute(1, 2, 0).contiguous())
        return [t.flip(0) if self.backward else t for t in out]


def _exact(got, want, what):
    got, want = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    bad = ~((got == want) | (got.isnan() & want.isnan()))
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference; first at flat index {i}: "
                             f"kernel {got[i].item()!r}, reference {want[i].item()!r}")


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("B,S", Q.RNN_LATTICE_CASES)
def test_rnn_lattice_is_bit_exact(dev, B, S, backward):
    ops, want, st = _reference(Q.rnn_lattice_case, B, S, backward)
    who = f"rnn lattice B {B} S {S} {'backward' if backward else 'forward'}"
    sw = _Sweep(dev, S, B, ops, backward, wpad=64 if (B + S) % 2 else 0)
    z16, z16t = sw.run()
    assert (z16t is not None) == (B % 8 == 0)
    # every row outside 0 .. S+1 and the gap after each wave step's B rows keep their sentinels; inside, zero_edges cleared row 0 and the
    # first half of row S+1 (both zero in the reference) and the sweep wrote the rest
    sw.z.assert_guards(who)
    got = sw.rows()
    _exact(got, want.float(), f"{who} state rows")
    assert not got[0].any() and not got[S + 1, :, :H].any() and not got[1, :, H:].any()
    mirrors = sw.mirrors(z16, z16t)
    for t, name in zip(mirrors, ("bf16 mirror", "transposed bf16 mirror")):
        t, w16 = t.clone(), got.to(BF16)
        t[S + 1, :, :H] = 0                                           # the half of the sweep's last row that is never produced (never read either)
        _exact(t, w16, f"{who} {name}")
    first = got.clone()
    z16b, z16tb = sw.run()                                            # the buffer now holds finite values: zero_edges and the sweep rewrite them
    sw.z.assert_guards(f"{who} replay")
    same_bits(first, sw.rows(), who)
    for a, b in zip(mirrors, sw.mirrors(z16b, z16tb)):
        a, b = a.clone(), b.clone()
        a[S + 1, :, :H] = 0
        b[S + 1, :, :H] = 0
        same_bits(a, b, f"{who} mirrors")


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("B,S", Q.RNN_RANDOM_CASES)
def test_rnn_random_against_float64(dev, B, S, backward):
    ops, plain, e32, _ = _reference(Q.rnn_random_case, B, S, backward)
    mode = "backward" if backward else "forward"
    sw = _Sweep(dev, S, B, ops, backward, sentinel=False)             # a zero-initialised buffer without zero_edges, as the per-step callers had
    sw.run()
    sw.z.assert_guards(f"rnn {mode} B {B} S {S}")
    got = sw.rows()
    assert not got[0].any() and not got[S + 1, :, :H].any() and not got[1, :, H:].any()
    compare_rows(f"rnn_wavefront {mode}", f"B{B} S{S}", Q.rnn_rows(got, S), Q.rnn_rows(plain, S), Q.rnn_rows(e32, S), MARGIN[mode])
    first = got.clone()
    sw.run()
    same_bits(first, sw.rows(), f"rnn {mode} B {B} S {S}")


def test_rnn_refusals(dev):
    S, B = 2, 3
    ops, _, _ = _reference(Q.rnn_lattice_case, B, S, False)
    sw = _Sweep(dev, S, B, ops, False)                                # sentinel-filled state buffer, zero_edges on
    size = "hulc_rnn_wavefront: needs 1 <= B <= 64 rows and S >= 1"
    refused(lambda: sw.run(H=1024), "hulc_rnn_wavefront: built for hidden size 2048", sw.z)
    refused(lambda: sw.run(B=0), size, sw.z)
    refused(lambda: sw.run(B=65), size, sw.z)
    refused(lambda: sw.run(S=0), size, sw.z)
    odd = torch.zeros(H * (H + 8) + 8, dtype=BF16, device=dev)[1:1 + H * (H + 8)].view(H, H + 8)[:, :H]      # 2 bytes off a 16-byte boundary
    refused(lambda: sw.run(w=[sw.w[0], odd, sw.w[2]]), "hulc_rnn_wavefront: k-major weights must be 16-byte aligned", sw.z)
    pitch = torch.zeros(H, H + 4, dtype=BF16, device=dev)[:, :H]                                             # rows 8 bytes apart from alignment
    refused(lambda: sw.run(w=[pitch, sw.w[1], sw.w[2]]), "hulc_rnn_wavefront: k-major weights must be 16-byte aligned", sw.z)
    refused(lambda: sw.run(w=[sw.w[0].float(), sw.w[1], sw.w[2]]), "weights must be bf16", sw.z)


@pytest.mark.parametrize("layouts", [(False, True, False), (True, True, False), (False, False, True)])
def test_rnn_refuses_mixed_layouts_before_it_clears_anything(dev, layouts):
    """zero_edges clears row 0 and half of row S+1 in a launch of its own ahead of the sweep: a call refused for its weight layouts must not
    have got that far"""
    S, B = 2, 3
    ops, _, _ = _reference(Q.rnn_lattice_case, B, S, False)
    sw = _Sweep(dev, S, B, ops, False)
    refused(lambda: sw.run(transposed=layouts), "hulc_rnn_wavefront: the three weight matrices share one layout", sw.z)
