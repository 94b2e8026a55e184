"""Kernel-level tests of the paired mode of csrc/rnn_wavefront.hip: kn.rnn_wavefront_pair called directly, against birnnref.pair_sweep, the
recurrence exactly as include/hulc2_amd.h states it (tests/test_birnn_cpu.py ties that reference to seqref.rnn_sweep and to nn.RNN).  Laid out
like tests/test_rnn_kernel_gpu.py, whose helpers it borrows:

  * the state buffer is TIME-ALIGNED, as the BiRNN posterior uses it: S + 2 sentinel-filled rows (with a gap of one state row after the B rows
    of each), row t + 1 = [first half at time t | second half at time t], while the two halves walk time in OPPOSITE directions: the second
    half has a base and a step of its own for its fp32 rows, its mirror rows, add2 and mask2.  Forward mode = relu, add1 / add2, add1c /
    add2c, four biases, row-major weights, the first half walking up; backward mode = masks read out of a time-aligned (S + 2, B, 2H)
    activation buffer with opposite steps, transposed weights, the first half walking down;
  * exact cases: integer lattices (birnnref.pair_lattice) — every written state row and the bf16 mirror equal the float64 emulation BIT FOR
    BIT, zero_edges clears exactly the row at z0, everything else keeps its sentinels, and a second launch reproduces the bits;
  * random cases at the model's magnitudes, per (wave step, batch row, half), under the bar of the existing sweeps;
  * the solo sweep (wB2 = None): the first half bit for bit the paired launch's, the second half's columns untouched;
  * refusals, none of which may launch anything.
Every launch is followed by kn.check_faults (the kernel's device-wide barrier reports a timeout there)."""
import functools
import time

import pytest
import torch

from tests import birnnref as R
from tests import kcheck as K
from tests.kcheck import Guarded, compare_rows, refused, same_bits
from tests.test_rnn_kernel_gpu import MARGIN, _exact, _padded, _reference

pytestmark = pytest.mark.gpu

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
    K.report("tests/test_rnn_pair_kernel_gpu.py")
    print(f"[kcheck-time] tests/test_rnn_pair_kernel_gpu.py {time.time() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def _lattice(B, S, backward):
    return _reference(R.pair_lattice_case, B, S, backward)


@functools.lru_cache(maxsize=None)
def _random(B, S, backward):
    return _reference(R.pair_random_case, B, S, backward)


class _Pair:
    """one paired sweep's operands on the device in the time-aligned layout: buffer row t + 1 holds time t of both halves.  Forward mode: the
    first half is at time tau at wave step tau, the second at time S - 1 - tau; backward mode: the other way round."""

    def __init__(self, dev, S, B, ops, backward, wpad=64, solo=False):
        from hulc2_amd import kernels as kn

        kn.set_compute("bf16")
        self.dev, self.S, self.B, self.backward, self.solo = dev, S, B, backward, solo
        self.w = [_padded(dev, ops[n].t().contiguous() if backward else ops[n], wpad, BF16) for n in ("wA", "wB2")]
        self.ld_z = B * 2 * H + 2 * H                                  # one state row of gap after every wave step's B rows
        self.z = Guarded(dev, S + 2, B * 2 * H, ld=self.ld_z)
        self.before = self.z.value()                                   # the sentinels
        kw = dict(relu=bool(ops.get("relu")), zero_edges=True)
        # the external terms in TIME order; the half that walks time backwards reads them from the far end with a negative step
        up, down = ("add2", "add1") if backward else ("add1", "add2")  # which operand walks up / down the buffer
        self.add_up, self.add_down = _padded(dev, ops[up], 8), _padded(dev, ops[down].flip(0), 8)
        for name, t, first, sign in ((up, self.add_up, 0, 1), (down, self.add_down, S - 1, -1)):
            kw.update({name: t[first], name + "_step": sign * t.stride(0), "ld_" + name: t.stride(1)})
        if backward:
            # masks: the stored activations of a forward pass, time-aligned (S + 2, B, 2H) rows of pitch 2H; everything else NaN (never kept)
            m = torch.full((S + 2, B, 2 * H), float("nan"), dtype=torch.float64)
            for tau in range(S):
                m[S - tau, :, :H] = ops["mask1"][tau]
                m[tau + 1, :, H:] = ops["mask2"][tau]
            self.m = m.to(dev, F32)
            kw.update(mask1=self.m[S, :, :H], mask1_step=-B * 2 * H, ld_mask1=2 * H, mask2=self.m[1, :, H:], mask2_step=B * 2 * H, ld_mask2=2 * H)
            self.z0, self.z_step = self.z.t[S + 1], -self.ld_z
            kw.update(z2=self.z.t[1], z2_step=self.ld_z, mirror2_row0=1, mirror2_step=1)
        else:
            self.z0, self.z_step = self.z.t[0], self.ld_z
            kw.update(z2=self.z.t[S], z2_step=-self.ld_z, mirror2_row0=S, mirror2_step=-1)
        for name in ("add1c", "add2c"):
            if ops.get(name) is not None:
                setattr(self, name, _padded(dev, ops[name], 16))
                kw[name] = getattr(self, name)
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
        z16 = kn.rnn_wavefront_pair(self.z0, self.z_step, a["S"], a["B"], a["H"], w[0], None if self.solo else w[1],
                                    self.backward if transposed is None else transposed, **{**self.kw, **override})
        torch.cuda.synchronize()
        kn.check_faults(self.dev)
        return z16.clone()

    def buffer(self):
        """the fp32 buffer (S + 2, B, 2H) in buffer (= time) order"""
        return self.z.value().view(self.S + 2, self.B, 2 * H)

    def expected(self, want):
        """the buffer a sweep must leave, from the rows `want` (S + 1, B, 2H) in sweep order: sentinels where nothing is written"""
        S = self.S
        e = self.before.view(S + 2, self.B, 2 * H).clone()
        e[S + 1 if self.backward else 0] = 0                           # zero_edges: the row at z0
        down, up = want[1:].flip(0).to(e), want[1:].to(e)              # rows 1 .. S of the buffer for the half that walks down / up
        e[1:S + 1, :, :H] = (down if self.backward else up)[:, :, :H]
        if not self.solo:
            e[1:S + 1, :, H:] = (up if self.backward else down)[:, :, H:]
        return e

    def rows(self):
        """the fp32 state rows in SWEEP order (S + 1, B, 2H): row 0 = the row at z0"""
        S, b = self.S, self.buffer()
        z = torch.empty(S + 1, self.B, 2 * H, dtype=F32, device=b.device)
        z[0] = b[S + 1 if self.backward else 0]
        z[1:, :, :H] = b[1:S + 1, :, :H].flip(0) if self.backward else b[1:S + 1, :, :H]
        z[1:, :, H:] = b[1:S + 1, :, H:] if self.backward else b[1:S + 1, :, H:].flip(0)
        return z


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("B,S", R.PAIR_LATTICE_CASES)
def test_pair_lattice_is_bit_exact(dev, B, S, backward):
    ops, want, st = _lattice(B, S, backward)
    who = f"pair lattice B {B} S {S} {'backward' if backward else 'forward'}"
    assert st["nonzero"] > 0.05, f"{who}: a dead lattice ({st})"
    sw = _Pair(dev, S, B, ops, backward, wpad=64 if (B + S) % 2 else 0)
    z16 = sw.run()
    sw.z.assert_guards(who)
    got, exp = sw.buffer(), sw.expected(want)
    assert torch.equal(_bits(got[[0, S + 1]]), _bits(exp[[0, S + 1]])), f"{who}: the rows at either end (zeros at z0, sentinels at the other)"
    _exact(got[1:S + 1], exp[1:S + 1], f"{who} state rows")
    _exact(z16[1:S + 1], got[1:S + 1].to(BF16), f"{who} bf16 mirror")
    assert not z16[S + 1 if backward else 0].any(), f"{who}: the mirror's initial region"
    z16b = sw.run()                                                    # the buffer now holds finite values: the sweep rewrites them
    sw.z.assert_guards(f"{who} replay")
    same_bits(_bits(got), _bits(sw.buffer()), who)                    # (as bit patterns: the row nobody writes holds NaN sentinels)
    same_bits(z16[1:S + 1], z16b[1:S + 1], f"{who} mirror")


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("B,S", R.PAIR_RANDOM_CASES)
def test_pair_random_against_float64(dev, B, S, backward):
    ops, plain, e32, _ = _random(B, S, backward)
    mode = "backward" if backward else "forward"
    sw = _Pair(dev, S, B, ops, backward)
    sw.run()
    sw.z.assert_guards(f"pair {mode} B {B} S {S}")
    got = sw.rows()
    assert not got[0].any()
    compare_rows(f"rnn_wavefront_pair {mode}", f"B{B} S{S}", R.pair_rows(got), R.pair_rows(plain), R.pair_rows(e32), MARGIN[mode])
    first = got.clone()
    sw.run()
    same_bits(first, sw.rows(), f"pair {mode} B {B} S {S}")


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("B,S", [(7, 2), (33, 3), (64, 8)])
def test_solo_sweep_is_the_first_half_alone(dev, B, S, backward):
    """wB2 = None: the first half's bits are the paired launch's (the lattice's expected rows), and no element of the second half's columns
    is written, in rows 1 .. S or anywhere else"""
    ops, want, _ = _lattice(B, S, backward)
    who = f"solo B {B} S {S} {'backward' if backward else 'forward'}"
    pair = _Pair(dev, S, B, ops, backward)
    pair.run()
    sw = _Pair(dev, S, B, ops, backward, solo=True)
    z16 = sw.run()
    sw.z.assert_guards(who)
    got = sw.buffer()
    assert torch.equal(_bits(got), _bits(sw.expected(want))), f"{who}: first half, or a write outside it"
    same_bits(got[1:S + 1, :, :H], pair.buffer()[1:S + 1, :, :H], who)
    _exact(z16[1:S + 1, :, :H], got[1:S + 1, :, :H].to(BF16), f"{who} bf16 mirror")


def test_pair_refusals(dev):
    S, B = 2, 3
    ops, _, _ = _reference(R.pair_lattice, S, B, 1, False)
    sw = _Pair(dev, S, B, ops, False)                                  # sentinel-filled state buffer, zero_edges on
    size = "hulc_rnn_wavefront_pair: needs 1 <= B <= 64 rows and S >= 1"
    refused(lambda: sw.run(H=1024), "hulc_rnn_wavefront_pair: built for hidden size 2048", sw.z)
    refused(lambda: sw.run(B=0), size, sw.z)
    refused(lambda: sw.run(B=65), size, sw.z)
    refused(lambda: sw.run(S=0), size, sw.z)
    for layouts in ((False, False, True), (True, True, False)):       # (wA, unused, wB2)
        refused(lambda: sw.run(transposed=layouts), "hulc_rnn_wavefront_pair: the two weight matrices share one layout", sw.z)
    odd = torch.zeros(H * (H + 8) + 8, dtype=BF16, device=dev)[1:1 + H * (H + 8)].view(H, H + 8)[:, :H]      # 2 bytes off a 16-byte boundary
    refused(lambda: sw.run(w=[sw.w[0], odd]), "hulc_rnn_wavefront_pair: k-major weights must be 16-byte aligned", sw.z)
    pitch = torch.zeros(H, H + 4, dtype=BF16, device=dev)[:, :H]                                             # rows 8 bytes apart from alignment
    refused(lambda: sw.run(w=[pitch, sw.w[1]]), "hulc_rnn_wavefront_pair: k-major weights must be 16-byte aligned", sw.z)
    refused(lambda: sw.run(w=[sw.w[0].float(), sw.w[1]]), "weights must be bf16", sw.z)
    refused(lambda: sw.run(z2=None), "hulc_rnn_wavefront_pair: null pointer (z2)", sw.z)
    refused(lambda: sw.run(mirror2_row0=S + 2), "hulc_rnn_wavefront_pair: mirror_row0 + tau * mirror_step must stay in 0 .. S+1", sw.z)
    refused(lambda: sw.run(mirror2_row0=0), "hulc_rnn_wavefront_pair: mirror_row0 + tau * mirror_step must stay in 0 .. S+1", sw.z)   # 0 - (S - 1) < 0
