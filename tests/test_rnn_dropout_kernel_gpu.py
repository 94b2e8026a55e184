"""Kernel-level tests of the decoder RNN's inter-layer dropout: kn.rnn_wavefront_drop and kn.rnn_drop_rows called directly, against
tests/rnndropref.py (seqref's sweep with the two masked modes; tests/test_rnn_dropout_cpu.py checks it against torch's nn.RNN(dropout=p)).
The sweeps are laid out as tests/test_rnn_kernel_gpu.py lays them out: padded NaN-filled operands, a sentinel-filled state buffer with a gap
after every wave step's rows.

  * exact: seqref's integer lattice with p = 0.5 (scale 2): state rows and bf16 mirrors equal the float64 emulation under the counter-RNG mask
    BIT FOR BIT, both modes, guards intact, a second launch bit-identical;
  * random operands at the model's magnitudes, p = 0.1, per (wave step, batch row, half) under the bar of tests/test_rnn_kernel_gpu.py;
  * p = 0 through the new entry has the bits of kn.rnn_wavefront; p outside [0, 1) is refused with nothing launched;
  * hulc_rnn_drop_rows bit for bit against x * counter_rng.dropout_scale.
Every sweep is followed by kn.check_faults (the kernel's device-wide barrier reports a timeout there)."""
import time

import numpy as np
import pytest
import torch

from oracle import counter_rng as R
from tests import kcheck as K
from tests import rnndropref as D
from tests import seqref as Q
from tests.kcheck import Guarded, compare_rows, refused, same_bits
from tests.test_rnn_kernel_gpu import MARGIN, _Sweep, _exact, _reference

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
    K.report("tests/test_rnn_dropout_kernel_gpu.py")
    print(f"[kcheck-time] tests/test_rnn_dropout_kernel_gpu.py {time.time() - t0:.1f} s")


@pytest.fixture(autouse=True)
def _word(dev):
    """the device RNG word the references were drawn with; the default word afterwards"""
    from hulc2_amd import kernels as kn

    kn.reset_step_state(dev, seed=D.RNG_WORD)
    yield
    kn.reset_step_state(dev)


class _DropSweep(_Sweep):
    """_Sweep through hulc_rnn_wavefront_drop: the forward sweep masks the wB1 product's inputs at t = tau - 1, the backward sweep its outputs
    at t = S - tau"""

    def run(self, p, site=D.DECODER_RNN_SITE, **override):
        from hulc2_amd import kernels as kn

        S = override.pop("S", self.S)
        mode, t0, t_dir = (kn.RNN_DROP_N, S, -1) if self.backward else (kn.RNN_DROP_K, -1, 1)
        z16, z16t = kn.rnn_wavefront_drop(self.z0, self.z_step, S, self.B, H, self.w[0], self.w[1], self.w[2], self.backward,
                                          p, site, override.pop("mode", mode), override.pop("t0", t0), override.pop("t_dir", t_dir),
                                          **{**self.kw, **override})
        torch.cuda.synchronize()
        kn.check_faults(self.dev)
        return z16, z16t


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("B,S", D.LATTICE_CASES)
def test_rnn_dropout_lattice_is_bit_exact(dev, B, S, backward):
    ops, keep, want = _reference(D.lattice_case, B, S, backward)
    who = f"rnn dropout lattice B {B} S {S} {'backward' if backward else 'forward'}"
    assert 0 < int((keep == 0).sum()) < keep.numel()
    sw = _DropSweep(dev, S, B, ops, backward, wpad=64 if (B + S) % 2 else 0)
    z16, z16t = sw.run(D.LATTICE_P)
    assert (z16t is not None) == (B % 8 == 0)
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
    z16b, z16tb = sw.run(D.LATTICE_P)
    sw.z.assert_guards(f"{who} replay")
    same_bits(first, sw.rows(), who)
    for a, b in zip(mirrors, sw.mirrors(z16b, z16tb)):
        a, b = a.clone(), b.clone()
        a[S + 1, :, :H] = 0
        b[S + 1, :, :H] = 0
        same_bits(a, b, f"{who} mirrors")


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("B,S", D.RANDOM_CASES)
def test_rnn_dropout_random_against_float64(dev, B, S, backward):
    ops, keep, plain, e32 = _reference(D.random_case, B, S, backward)
    mode = "backward" if backward else "forward"
    sw = _DropSweep(dev, S, B, ops, backward, sentinel=False)
    sw.run(D.RANDOM_P)
    sw.z.assert_guards(f"rnn dropout {mode} B {B} S {S}")
    got = sw.rows()
    assert not got[0].any() and not got[S + 1, :, :H].any() and not got[1, :, H:].any()
    compare_rows(f"rnn_wavefront_drop {mode}", f"B{B} S{S}", Q.rnn_rows(got, S), Q.rnn_rows(plain, S), Q.rnn_rows(e32, S), MARGIN[mode])
    first = got.clone()
    sw.run(D.RANDOM_P)
    same_bits(first, sw.rows(), f"rnn dropout {mode} B {B} S {S}")


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_zero_probability_is_the_plain_sweep(dev, backward):
    B, S = 7, 2
    ops, _, _ = _reference(Q.rnn_lattice_case, B, S, backward)
    plain = _Sweep(dev, S, B, ops, backward)
    z16, _ = plain.run()
    drop = _DropSweep(dev, S, B, ops, backward)
    d16, _ = drop.run(0.0)
    drop.z.assert_guards("p = 0")
    same_bits(plain.rows(), drop.rows(), "p = 0 through hulc_rnn_wavefront_drop")
    a, b = z16.clone(), d16.clone()
    a[S + 1 if not backward else 0, :, :H] = 0
    b[S + 1 if not backward else 0, :, :H] = 0
    same_bits(a, b, "p = 0 through hulc_rnn_wavefront_drop, bf16 mirror")


def test_refusals_launch_nothing(dev):
    S, B = 2, 3
    ops, _, _ = _reference(Q.rnn_lattice_case, B, S, False)
    sw = _DropSweep(dev, S, B, ops, False)                            # sentinel-filled state buffer, zero_edges on
    refused(lambda: sw.run(1.0), "hulc_rnn_wavefront_drop: drop_p must be in [0, 1)", sw.z)
    refused(lambda: sw.run(-0.1), "hulc_rnn_wavefront_drop: drop_p must be in [0, 1)", sw.z)
    refused(lambda: sw.run(0.1, mode=3), "hulc_rnn_wavefront_drop: mode is HULC_RNN_DROP_K or HULC_RNN_DROP_N", sw.z)
    refused(lambda: sw.run(0.1, t0=0), "hulc_rnn_wavefront_drop: t0 + tau * t_dir must stay in 0 .. S-1", sw.z)
    refused(lambda: sw.run(0.1, t_dir=2), "hulc_rnn_wavefront_drop: t0 + tau * t_dir must stay in 0 .. S-1", sw.z)
    refused(lambda: sw.run(0.1, S=0), "hulc_rnn_wavefront: needs 1 <= B <= 64 rows and S >= 1", sw.z)


@pytest.mark.parametrize("row0", [0, 3])
@pytest.mark.parametrize("Hd", [2048, 96])
@pytest.mark.parametrize("rows", [5, 33])
def test_drop_rows_is_bit_exact(dev, rows, Hd, row0):
    from hulc2_amd import kernels as kn

    p, site = 0.1, D.MODALITY_SITES["lang"]
    g = torch.Generator().manual_seed(1000 * rows + Hd + row0)
    x = torch.randn(rows, Hd, generator=g)
    xbuf = torch.full((rows, Hd + 24), float("nan"), device=dev)      # pitch larger than H; a read outside the view poisons the result
    xv = xbuf[:, :Hd]
    xv.copy_(x)
    idx = (np.arange(rows * Hd, dtype=np.uint64) + np.uint64(row0 * Hd)).reshape(rows, Hd)
    scale = R.dropout_scale(site ^ D.RNG_WORD, idx, p)
    assert 0 < int((scale == 0).sum()) < scale.size
    want = torch.from_numpy(x.numpy() * scale)                        # one fp32 rounding: the product of an fp32 value and {0, fp32(1 / (1 - p))}
    o32, o16 = Guarded(dev, rows, Hd, F32, ld=Hd + 8), Guarded(dev, rows, Hd, BF16, ld=Hd + 40)
    kn.rnn_drop_rows(xv, rows, Hd, row0, p, site, out32=o32.t, out16=o16.t)
    torch.cuda.synchronize()
    o32.assert_guards("drop_rows fp32")
    o16.assert_guards("drop_rows bf16")
    _exact(o32.value(), want, f"drop_rows fp32 rows {rows} H {Hd} row0 {row0}")
    _exact(o16.value(), want.to(BF16), f"drop_rows bf16 rows {rows} H {Hd} row0 {row0}")
    only16 = Guarded(dev, rows, Hd, BF16, ld=Hd + 8)                  # one destination at a time
    kn.rnn_drop_rows(xv, rows, Hd, row0, p, site, out16=only16.t)
    only32 = Guarded(dev, rows, Hd, F32, ld=Hd + 16)
    kn.rnn_drop_rows(xv, rows, Hd, row0, p, site, out32=only32.t)
    torch.cuda.synchronize()
    only16.assert_guards("drop_rows bf16 alone")
    only32.assert_guards("drop_rows fp32 alone")
    same_bits(only16.value(), o16.value(), "drop_rows bf16 alone")
    same_bits(only32.value(), o32.value(), "drop_rows fp32 alone")


def test_drop_rows_refusals(dev):
    from hulc2_amd import kernels as kn

    x = torch.zeros(4, 96, device=dev)
    out = Guarded(dev, 4, 96, F32)
    refused(lambda: kn.rnn_drop_rows(x, 4, 96, 0, 1.0, 1, out32=out.t), "hulc_rnn_drop_rows: drop_p must be in [0, 1)", out)
    refused(lambda: kn.rnn_drop_rows(x[:, :94], 4, 94, 0, 0.1, 1, out32=out.t), "hulc_rnn_drop_rows: needs rows >= 0, H a positive multiple of 4", out)
    refused(lambda: kn.rnn_drop_rows(x, 4, 96, 0, 0.1, 1), "hulc_rnn_drop_rows: null pointer", out)
