"""Kernel-level tests of the attention half (csrc/txl_fused.hip, csrc/txl_attn.h): kn.txl_attn_fwd / kn.txl_attn_bwd called directly, every
output the descriptor names checked on its own against the float64 references of tests/seqref.py.

  * exact forward cases in which softmax is exact (seqref.attn_lattice: one key; uniform attention over a power of two of keys;
    permutation attention onto a non-identity, non-involutive target) on integer x, Wv, Wo: the kept tensors ctx and pre must equal the
    float64 emulation BIT FOR BIT, with and without dropout 0.5; y / mean / rstd are the LayerNorm of an exactly known pre and are held to
    the float32 CPU LayerNorm's error times LIBM;
  * exact backward cases from pre = 0, mean = 0, rstd = 1 and integer dy (+ 0, 1, 4, 5 or 16 integer slabs with a pitch of their own):
    d_o, dqkv, dx and ln_partial bit for bit;
  * random cases at the model's magnitudes against the plain float64 reference, per token / per sequence (kcheck.compare_rows);
  * sequence independence of every output; refusals.
The pattern of a case (guard bands, replay, refusals) is that of tests/kcheck.py."""
import time

import pytest
import torch
import torch.nn.functional as F

from tests import kcheck as K
from tests import seqref as Q
from tests.kcheck import Guarded, compare, compare_rows, out_flat, refused, same_bits

pytestmark = pytest.mark.gpu

# LIBM 4: value and meaning of tests/test_losses_gpu.py (kcheck.compare: max-abs over max-abs, yardstick = the float32 CPU formula): the
#         LayerNorm of an exactly known input, where only summation order, fused multiply-adds and rsqrtf differ.
# The others: margin * max(e_ref, 2^-23) per row (kcheck.compare_rows), e_ref = the CPU emulation of the kernel's bf16 rounding points
#         with float32 arithmetic.  Kernel and emulation share the rounding points and differ in fp32 summation order and in the exponential.
MARGIN = {"LIBM": 4.0, "y": 2.0, "pre": 2.0, "mean": 2.0, "rstd": 2.0, "ctx": 2.0, "dx": 2.0, "d_o": 2.0, "dqkv": 2.0, "ln_partial": 2.0}

BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-5
REFUSED_FWD = "hulc_txl_attn_fwd: needs d_model 128, 8 heads, 1 <= S <= 32 and non-null operands"
REFUSED_BWD = "hulc_txl_attn_bwd: needs d_model 128, 8 heads, 1 <= S <= 32 and non-null operands"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    K.report("tests/test_txl_attn_kernel_gpu.py")
    print(f"[kcheck-time] tests/test_txl_attn_kernel_gpu.py {time.time() - t0:.1f} s")


def _reference(build, *args):
    """the CPU references on at most 8 threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(8, n))
    try:
        return build(*args)
    finally:
        torch.set_num_threads(n)


class _Layer:
    """the operands of one attention half on the device and guarded outputs for both directions"""

    def __init__(self, dev, ops, p):
        from hulc2_amd import kernels as kn

        kn.set_compute("bf16")
        self.dev, self.B, self.S, self.p = dev, ops["B"], ops["S"], p
        self.T = self.B * self.S
        up = lambda name, dt: self._exact_copy(ops[name], dt, name)
        self.x = up("x", F32)
        self.Wqkv, self.Wo = up("Wqkv", BF16), up("Wo", BF16)
        self.WqkvT, self.WoT = self.Wqkv.t().contiguous(), self.Wo.t().contiguous()
        self.bqkv, self.bo, self.gamma, self.beta = up("bqkv", F32), up("bo", F32), up("gamma", F32), up("beta", F32)
        if p > 0.0:
            kn.reset_step_state(dev, seed=Q.RNG_WORD)
            assert int(kn.step_state(dev)[0].item()) == Q.RNG_WORD
        T = self.T
        self.y, self.pre, self.ctx = Guarded(dev, T, Q.E), Guarded(dev, T, Q.E), Guarded(dev, T, Q.E, BF16)
        self.mean, self.rstd = out_flat(dev, T), out_flat(dev, T)
        self.dx, self.d_o, self.dqkv = Guarded(dev, T, Q.E), Guarded(dev, T, Q.E, BF16), Guarded(dev, T, 3 * Q.E, BF16)
        self.ln_partial = Guarded(dev, self.B * 2, Q.E)

    def _exact_copy(self, t64, dt, name):
        t = t64.to(self.dev, dt)
        assert torch.equal(t.double().cpu(), t64), f"{name} is not exact in its storage type"
        return t

    def fwd(self, keep=True, y=None, **over):
        from hulc2_amd import kernels as kn

        a = dict(B=self.B, S=self.S, H=Q.NH)
        a.update(over)
        kept = dict(pre=self.pre.t, mean=self.mean.t, rstd=self.rstd.t, ctx=self.ctx.t) if keep is True else (keep or {})
        kn.txl_attn_fwd(self.x, self.Wqkv, self.bqkv, self.Wo, self.bo, self.gamma, self.beta, EPS, a["B"], a["S"], a["H"], self.p,
                        Q.ATTN_SEEDS[0], Q.ATTN_SEEDS[1], (y or self.y).t, **kept)
        torch.cuda.synchronize()

    def set_bwd(self, bops):
        """the backward's inputs: kept tensors, dy and the partial slabs, (n, T E) at a pitch of T E + 256 inside a NaN-filled allocation"""
        self.bpre, self.bmean, self.brstd = (self._exact_copy(bops[k], F32, k) for k in ("pre", "mean", "rstd"))
        self.dy = self._exact_copy(bops["dy"], F32, "dy")
        n = bops["slabs"].shape[0]
        self.n_slab, self.slab_stride = n, self.T * Q.E + 256
        self.slabs = None
        if n:
            buf = torch.full((n, self.slab_stride), float("nan"), dtype=F32, device=self.dev)
            buf[:, :self.T * Q.E] = bops["slabs"].reshape(n, -1).to(self.dev, F32)
            assert torch.equal(buf[:, :self.T * Q.E].double().cpu(), bops["slabs"].reshape(n, -1))
            self.slabs = buf

    def bwd(self, ln_partial=None, **over):
        from hulc2_amd import kernels as kn

        a = dict(B=self.B, S=self.S, H=Q.NH)
        a.update(over)
        kn.txl_attn_bwd(self.x, self.Wqkv, self.WqkvT, self.WoT, self.bqkv, self.gamma, EPS, a["B"], a["S"], a["H"], self.p, Q.ATTN_SEEDS[0],
                        Q.ATTN_SEEDS[1], self.bpre, self.bmean, self.brstd, self.dy, self.slabs, self.n_slab, self.slab_stride, self.dx.t, self.d_o.t,
                        self.dqkv.t, self.ln_partial.t if ln_partial is None else ln_partial)
        torch.cuda.synchronize()

    def outputs(self, names):
        for n in names:
            getattr(self, n).assert_guards(n)
        return {n: getattr(self, n).value().reshape(self.T if n in ("mean", "rstd") else (self.B, 2, Q.E) if n == "ln_partial" else (self.T, -1))
                for n in names}


FWD, BWD = ("y", "pre", "mean", "rstd", "ctx"), ("dx", "d_o", "dqkv", "ln_partial")


def _exact(got, want64, what):
    got, want = got.detach().cpu().reshape(-1), want64.to(got.dtype).reshape(-1)
    assert torch.equal(want.double(), want64.reshape(-1)), f"{what}: the expected values are not {got.dtype} numbers (a broken lattice)"
    bad = got != want
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference; first at flat index {i}: "
                             f"kernel {got[i].item()!r}, reference {want[i].item()!r}")


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("kind,B,S", Q.ATTN_LATTICE_CASES)
def test_attention_lattice_is_bit_exact(dev, kind, B, S, p):
    n_slab = Q.attn_lattice_slabs(B, S, p)
    ops, fw, bops, bw, _ = _reference(Q.attn_lattice_case, kind, B, S, p, n_slab)
    who = f"attention {kind} B {B} S {S} p {p}"
    L = _Layer(dev, ops, p)
    # ---- forward: ctx and pre exact; y / mean / rstd = LayerNorm of the exactly known pre
    L.fwd()
    got = L.outputs(FWD)
    _exact(got["ctx"], fw["ctx"], f"{who} ctx")
    _exact(got["pre"], fw["pre"], f"{who} pre")
    pre32 = fw["pre"].float()
    mean32 = pre32.mean(-1)
    ref32 = dict(y=F.layer_norm(pre32, (Q.E,), ops["gamma"].float(), ops["beta"].float(), EPS), mean=mean32,
                 rstd=torch.rsqrt(((pre32 - mean32[:, None]) ** 2).mean(-1) + EPS))
    for name in ("y", "mean", "rstd"):
        compare("txl_attn_fwd layernorm", f"{name} {kind} B{B} S{S}", got[name], fw[name], ref32[name], MARGIN["LIBM"])
    L.fwd()
    for name, t in L.outputs(FWD).items():
        same_bits(got[name], t, f"{who} {name}")
    y2 = Guarded(dev, L.T, Q.E)
    L.fwd(keep=False, y=y2)                                           # inference: nothing kept, the same y
    y2.assert_guards(f"{who} y (nothing kept)")
    same_bits(got["y"], y2.value(), f"{who} y with pre = None")
    if bw is None:
        return
    # ---- backward from pre = 0, mean = 0, rstd = 1
    L.set_bwd(bops)
    L.bwd()
    gotb = L.outputs(BWD)
    for name in BWD:
        _exact(gotb[name], bw[name], f"{who} {name} ({n_slab} slabs)")
    L.bwd()
    for name, t in L.outputs(BWD).items():
        same_bits(gotb[name], t, f"{who} {name}")


@pytest.mark.parametrize("B,S,p,n_slab", Q.ATTN_RANDOM_CASES)
def test_attention_random_against_float64(dev, B, S, p, n_slab):
    ops, bops, plain, e32, _ = _reference(Q.attn_random_case, B, S, p, n_slab)
    who = f"B{B} S{S} p{p} n{n_slab}"
    L = _Layer(dev, ops, p)
    L.fwd()
    L.set_bwd(bops)                                                   # the kept operands are the reference's, rounded to fp32: backward on its own
    L.bwd()
    got = {**L.outputs(FWD), **L.outputs(BWD)}
    for name in Q.ATTN_OUTPUTS:
        compare_rows("txl_attn_fwd" if name in FWD else "txl_attn_bwd", f"{name} {who}", Q.attn_rows(name, got[name], B), Q.attn_rows(name, plain[name], B),
                     Q.attn_rows(name, e32[name], B), MARGIN[name])
    L.fwd()
    L.bwd()
    for name, t in {**L.outputs(FWD), **L.outputs(BWD)}.items():
        same_bits(got[name], t, f"{who} {name}")
    y2 = Guarded(dev, L.T, Q.E)
    L.fwd(keep=False, y=y2)
    same_bits(got["y"], y2.value(), f"{who} y with pre = None")


@pytest.mark.parametrize("B,S", [(3, 11), (100, 19)])
def test_attention_sequences_are_independent(dev, B, S):
    """S < 32: keys >= S are masked and rows >= S never stored, so changing sequences 1 .. leaves every output of sequence 0 bit-identical"""
    ops, bops, _, _, _ = _reference(Q.attn_random, B, S, 5, 0.1, Q.ATTN_SEEDS, Q.RNG_WORD, 4)
    results = []
    for trial in range(2):
        if trial:
            g = torch.Generator().manual_seed(99)
            for d, names in ((ops, ("x",)), (bops, ("dy", "pre", "mean", "rstd"))):
                for n in names:
                    d[n] = d[n].clone()
                    d[n][S:] = (torch.randn(d[n][S:].shape, generator=g, dtype=torch.float64) + (1.5 if n == "rstd" else 0.0)).float().double()
            bops["slabs"] = bops["slabs"].clone()
            bops["slabs"][:, S:] = torch.randn(bops["slabs"][:, S:].shape, generator=g, dtype=torch.float64).float().double()
        L = _Layer(dev, ops, 0.1)
        L.fwd()
        L.set_bwd(bops)
        L.bwd()
        results.append({**L.outputs(FWD), **L.outputs(BWD)})
    for name in Q.ATTN_OUTPUTS:
        a, b = results[0][name], results[1][name]
        assert not torch.equal(a, b), f"{name}: the other sequences did not change at all (a broken test)"
        n0 = 1 if name == "ln_partial" else S
        assert torch.equal(a[:n0], b[:n0]), f"{name}: sequence 0 changed with the other sequences"


def test_attention_refusals(dev):
    ops, fw, bops, _, _ = _reference(Q.attn_lattice_case, "perm", 3, 7, 0.0, 1)
    L = _Layer(dev, ops, 0.0)
    L.set_bwd(bops)
    fwd_out, bwd_out = [getattr(L, n) for n in FWD], [getattr(L, n) for n in BWD]
    for over in (dict(S=0), dict(S=33), dict(H=7), dict(H=16), dict(B=0)):
        refused(lambda: L.fwd(**over), REFUSED_FWD, *fwd_out)
        refused(lambda: L.bwd(**over), REFUSED_BWD, *bwd_out)
    together = "hulc_txl_attn_fwd: pre / mean / rstd are saved together or not at all"
    refused(lambda: L.fwd(keep=dict(pre=L.pre.t)), together, *fwd_out)
    refused(lambda: L.fwd(keep=dict(pre=L.pre.t, rstd=L.rstd.t)), together, *fwd_out)
    refused(lambda: L.fwd(keep=dict(mean=L.mean.t, rstd=L.rstd.t)), together, *fwd_out)
    null = torch.empty(0, dtype=F32, device=dev)                      # a tensor without storage: a null pointer for the launcher
    assert null.data_ptr() == 0
    refused(lambda: L.bwd(ln_partial=null), "hulc_txl_attn_bwd: null pointer", *bwd_out)
