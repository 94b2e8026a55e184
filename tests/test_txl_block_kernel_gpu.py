"""Kernel-level tests of the whole-trunk launches (csrc/txl_block.hip): kn.txl_block_desc + kn.txl_block_fwd / kn.txl_block_bwd called
directly, every kept tensor and every backward operand checked on its own against the float64 references of tests/seqref.py.

  * random cases at the model's magnitudes against the plain float64 reference with one row per SEQUENCE (kcheck.compare_rows), at shapes
    that reach every sharing factor (Q = 4, 2 and 1 workgroups per sequence, among them the natural Q = 1 above 128 sequences and an odd
    number of hidden slices per member), L = 1 .. 4, and position ids that are not arange(S);
  * exact cases where the trunk composes exactly: the position add with dropout 0.5 into layers[0].x, and with S = 1 layer 0's ctx / pre1;
  * bit equality between launch configurations that promise the same sums: Q = 4 against Q = 2 on the tensors ahead of the first exchange,
    packed against gathered feed-forward weights, every sequence of a batch against the same sequence launched alone;
  * sequence independence of every output; the split-operand forward against a float32 evaluation; refusals.
Every launch is followed by kn.check_faults (the shared-sequence exchange reports a timeout there)."""
import time

import pytest
import torch

from tests import kcheck as K
from tests import seqref as Q
from tests.kcheck import Guarded, compare_rows, refused, same_bits

pytestmark = pytest.mark.gpu

# margin * max(e_ref, 2^-23) per sequence, e_ref = the CPU emulation of the kernels' bf16 rounding points with float32 arithmetic.  Default 2
# for every tensor (kernel and emulation share the rounding points); entries here are the exceptions, each with its measured ratio and cause.
MARGIN = {}
DEFAULT_MARGIN = 2.0
# The split-operand forward against the float32 evaluation of the same formulas (test_split_operand_forward).  Every entry is above 2 for
# one cause: hi + lo = two bf16 keep 16 mantissa bits of an operand and the lo x lo term is dropped, so every product carries about 2^-17
# where float32 operands carry 2^-24; the rows come out at 3e-6 .. 5e-6 (1.4e-5 for the small mean1), the "fp32 class (~2^-16)" the header
# promises, against 1.5e-7 .. 2.5e-7 for float32 arithmetic.  Measured on an MI355X, largest ratio over both cases and all layers, each
# entry the next power of two above it: pre1 21.3 (B5 S7 L2 FF384, layer 0), pooled 20.1, pre2 19.9, y2 19.7, mean1 19.4, y1 19.4,
# mean2 11.1, rstd1 3.7, rstd2 2.02 (all B5 S7 L2 FF384, layer 1); x0 (no product) 0.23.
SPLIT_MARGIN = {"pre1": 32.0, "pooled": 32.0, "pre2": 32.0, "y2": 32.0, "mean1": 32.0, "y1": 32.0, "mean2": 16.0, "rstd1": 4.0, "rstd2": 4.0}

E, NH = Q.E, Q.NH
BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-5
REFUSED_FWD = "hulc_txl_block_fwd: needs d_model 128, 8 heads, 1 <= S <= 32, 1 <= L <= 4, FF a multiple of 128 and non-null operands"
REFUSED_BWD = "hulc_txl_block_bwd: needs d_model 128, 8 heads, 1 <= S <= 32, 1 <= L <= 4, FF a multiple of 128 and non-null operands"
FP32_KEPT = ("y1", "pre1", "mean1", "rstd1", "y2", "pre2", "mean2", "rstd2")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    K.report("tests/test_txl_block_kernel_gpu.py")
    print(f"[kcheck-time] tests/test_txl_block_kernel_gpu.py {time.time() - t0:.1f} s")


def _reference(build, *args):
    """the CPU references on at most 8 threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(8, n))
    try:
        return build(*args)
    finally:
        torch.set_num_threads(n)


def _packed(w_bf16, layout, FF):
    """fragment-packed copy of a feed-forward weight (hulc_ffn_frag_perm layouts 0: W1, 1: W2, 2: W2^T, 3: W1^T)"""
    from hulc2_amd import kernels as kn

    src = w_bf16 if layout in (0, 1) else w_bf16.t()
    perm = torch.from_numpy(kn.ffn_frag_perm(layout, FF)).to(device=w_bf16.device, dtype=torch.long)
    return src.contiguous().reshape(-1)[perm].contiguous()


class _Trunk:
    """one trunk's operands on the device, guarded outputs for both directions"""

    def __init__(self, dev, ops, p, packed=False, split=False, site=Q.TRUNK_SITE):
        from hulc2_amd import kernels as kn

        kn.set_compute("bf16")
        self.dev, self.p, self.site = dev, p, site
        self.B, self.S, _ = ops["emb"].shape
        self.L, self.FF = len(ops["layers"]), ops["layers"][0]["W1"].shape[0]
        self.T = self.B * self.S
        self.emb, self.pos = self._copy(ops["emb"], F32, "emb"), self._copy(ops["pos"], F32, "pos")
        self.pos_ids = ops["pos_ids"].to(dev)
        self.dpooled = self._copy(ops["dpooled"], F32, "dpooled")
        self.params = []
        for l in ops["layers"]:
            src = {n: l[n + "_hi"] if split and n[0] == "W" else l[n] for n in Q.LAYER_PARAMS}
            d = {n: self._copy(src[n], BF16 if n[0] == "W" else F32, n) for n in Q.LAYER_PARAMS}
            d.update({n + "T": d[n].t().contiguous() for n in ("Wqkv", "Wo", "W1", "W2")})
            if packed or split:
                d.update(W1p=_packed(d["W1"], 0, self.FF), W2p=_packed(d["W2"], 1, self.FF), W2Tp=_packed(d["W2"], 2, self.FF), W1Tp=_packed(d["W1"], 3, self.FF))
            if split:
                lo = {n: self._copy(l[n + "_lo"], BF16, n + "_lo") for n in ("Wqkv", "Wo", "W1", "W2")}
                d.update(Wqkv_lo=lo["Wqkv"], Wo_lo=lo["Wo"], W1p_lo=_packed(lo["W1"], 0, self.FF), W2p_lo=_packed(lo["W2"], 1, self.FF))
            self.params.append(d)
        if p > 0.0:
            kn.reset_step_state(dev, seed=Q.RNG_WORD)
            assert int(kn.step_state(dev)[0].item()) == Q.RNG_WORD
        T, B, FF = self.T, self.B, self.FF
        G = lambda rows, cols, dt=F32: Guarded(dev, rows, cols, dt)
        self.x0, self.pooled, self.demb = G(T, E), G(B, E), G(T, E)
        self.out = [dict(y1=G(T, E), pre1=G(T, E), mean1=G(1, T), rstd1=G(1, T), ctx=G(T, E, BF16), y2=G(T, E), pre2=G(T, E), mean2=G(1, T), rstd2=G(1, T),
                         d_o=G(T, E, BF16), dqkv=G(T, 3 * E, BF16), df=G(T, E, BF16), h=G(T, FF, BF16), dh=G(T, FF, BF16), lnp1=G(2 * B, E), lnp2=G(2 * B, E))
                    for _ in range(self.L)]

    def _copy(self, t64, dt, name):
        t = t64.to(self.dev, dt)
        assert torch.equal(t.double().cpu(), t64), f"{name} is not exact in its storage type"
        return t

    def records(self, backward, keep=True):
        recs, x = [], self.x0.t
        seeds = Q.trunk_seeds(self.site, self.L)
        for p, o, sd in zip(self.params, self.out, seeds):
            names = ["Wqkv", "Wo", "W1", "W2", "bqkv", "bo", "b1", "b2", "g1", "be1", "g2", "be2"]
            if backward:
                names += ["WqkvT", "WoT", "W1T", "W2T"] + [n for n in ("W1p", "W2Tp", "W1Tp") if n in p]
            else:
                names += [n for n in ("W1p", "W2p", "Wqkv_lo", "Wo_lo", "W1p_lo", "W2p_lo") if n in p]
            r = {n: p[n] for n in names}
            r.update(sd)
            r.update(x=x, y1=o["y1"].t, y2=o["y2"].t)
            if keep or backward:
                r.update({n: o[n].t for n in ("pre1", "mean1", "rstd1", "ctx", "pre2", "mean2", "rstd2")})
            if backward:
                r.update({n: o[n].t for n in Q.TRUNK_BWD})
            recs.append(r)
            x = o["y2"].t
        return recs

    def fwd(self, recs=None, B=None, S=None, H=NH, FF=None):
        from hulc2_amd import kernels as kn

        B, S, FF = B or self.B, S or self.S, FF or self.FF
        recs = self.records(False) if recs is None else recs
        d = kn.txl_block_desc(self.emb, self.pos, self.pos_ids, B, S, H, FF, self.p, self.site, EPS, recs, pooled=self.pooled.t)
        kn.txl_block_fwd(d, B, S, H, E, FF, len(recs))
        torch.cuda.synchronize()
        kn.check_faults(self.dev)

    def bwd(self, recs=None, **over):
        from hulc2_amd import kernels as kn

        recs = self.records(True) if recs is None else recs
        d = kn.txl_block_desc(self.emb, self.pos, self.pos_ids, self.B, self.S, NH, self.FF, self.p, self.site, EPS, recs,
                              dpooled=over.get("dpooled", self.dpooled), demb=over.get("demb", self.demb.t))
        kn.txl_block_bwd(d, self.B, self.S, NH, E, self.FF, len(recs))
        torch.cuda.synchronize()
        kn.check_faults(self.dev)

    def guards(self, forward_only=False):
        names = Q.TRUNK_KEPT if forward_only else Q.TRUNK_KEPT + Q.TRUNK_BWD
        return [self.x0, self.pooled] + ([] if forward_only else [self.demb]) + [o[n] for o in self.out for n in names]

    def results(self, forward_only=False):
        """{name: tensor} keyed as seqref.trunk_tensors"""
        for g in self.guards(forward_only):
            g.assert_guards("trunk")
        r = {"x0": self.x0.value(), "pooled": self.pooled.value()}
        if not forward_only:
            r["demb"] = self.demb.value()
        for li, o in enumerate(self.out):
            for n in (Q.TRUNK_KEPT if forward_only else Q.TRUNK_KEPT + Q.TRUNK_BWD):
                r[f"{li}.{n}"] = o[n].value()
        return r


def _seq(t, B, sl):
    """the rows of sequences `sl` of any trunk tensor"""
    return t.reshape(B, -1)[sl]


def _exact(got, want64, what):
    got, want = got.detach().cpu().reshape(-1), want64.to(got.dtype).reshape(-1)
    assert torch.equal(want.double(), want64.reshape(-1)), f"{what}: the expected values are not {got.dtype} numbers (a broken lattice)"
    bad = got != want
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference; first at flat index {i}: "
                             f"kernel {got[i].item()!r}, reference {want[i].item()!r}")


@pytest.mark.parametrize("B,S,L,FF", Q.TRUNK_RANDOM_CASES)
def test_trunk_random_against_float64(dev, B, S, L, FF):
    ops, plain, e32, _ = _reference(Q.trunk_random_case, B, S, L, FF)
    who = f"B{B} S{S} L{L} FF{FF}"
    t = _Trunk(dev, ops, Q.TRUNK_P)
    t.fwd()
    t.bwd()
    got = t.results()
    want, emu = dict(Q.trunk_tensors(plain)), dict(Q.trunk_tensors(e32))
    assert set(got) == set(want)
    for name in want:
        base = name.split(".")[-1]
        kernel = "txl_block_fwd" if base in Q.TRUNK_KEPT + ("x0", "pooled") else "txl_block_bwd"
        compare_rows(f"{kernel} Q={Q.TRUNK_SHARE[(B, S, L, FF)]}", f"{name} {who}", Q.trunk_rows(got[name], B), Q.trunk_rows(want[name], B),
                     Q.trunk_rows(emu[name], B), MARGIN.get(base, DEFAULT_MARGIN))
    t.fwd()
    t.bwd()
    for name, v in t.results().items():
        same_bits(got[name], v, f"{who} {name}")
    # the fragment-packed feed-forward weights hold the same values in another order of storage: the same products, the same sums
    tp = _Trunk(dev, ops, Q.TRUNK_P, packed=True)
    tp.fwd()
    tp.bwd()
    for name, v in tp.results().items():
        assert torch.equal(got[name], v), f"{who} {name}: packed and gathered feed-forward weights give different bits"
    # inference keeps nothing and gives the same pooled rows
    ti = _Trunk(dev, ops, Q.TRUNK_P)
    ti.fwd(recs=ti.records(False, keep=False))
    ti.pooled.assert_guards("pooled")
    for o in ti.out:
        for n in ("pre1", "mean1", "rstd1", "ctx", "pre2", "mean2", "rstd2"):
            o[n].assert_untouched(f"{who} {n} (inference)")
    same_bits(got["pooled"], ti.pooled.value(), f"{who} pooled (nothing kept)")


@pytest.mark.parametrize("B,S,L,FF", [(5, 19, 1, 128), (7, 1, 2, 256), (64, 1, 1, 2048)])
def test_trunk_exact_pieces(dev, B, S, L, FF):
    ops, exact = _reference(Q.trunk_lattice, B, S, L, FF, 11 * B + S, Q.TRUNK_SITE, Q.RNG_WORD)
    t = _Trunk(dev, ops, 0.5)
    t.fwd()
    got = t.results(forward_only=True)
    _exact(got["x0"], exact["x0"], f"B {B} S {S} layers[0].x = dropout(emb + pos[pos_ids])")
    assert (S == 1) == ("ctx" in exact)
    if S == 1:
        _exact(got["0.ctx"], exact["ctx"], f"B {B} layer 0 ctx")
        _exact(got["0.pre1"], exact["pre1"], f"B {B} layer 0 pre1")
    for v in got.values():
        assert torch.isfinite(v.float()).all()


def test_share_factors_agree_ahead_of_the_first_exchange(dev):
    """members of a shared sequence store identical values, and nothing ahead of the first exchange of partial tiles depends on the sharing
    factor: a B = 64 launch (Q = 4) and the same 64 sequences as the first half of a B = 128 launch (Q = 2) agree bit for bit in layers[0].x
    and the attention-half tensors of layer 0 (later layers sum 4 against 2 partial tiles and may differ)"""
    ops, _, _, _ = _reference(Q.trunk_random, 128, 32, 2, 2048, 5, Q.TRUNK_P, Q.TRUNK_SITE, Q.RNG_WORD, True)
    big = _Trunk(dev, ops, Q.TRUNK_P)
    big.fwd()
    half = dict(ops, emb=ops["emb"][:64], dpooled=ops["dpooled"][:64])
    small = _Trunk(dev, half, Q.TRUNK_P)
    small.fwd()
    a, b = big.results(forward_only=True), small.results(forward_only=True)
    for name in ("x0", "0.y1", "0.pre1", "0.mean1", "0.rstd1", "0.ctx"):
        assert torch.equal(_seq(a[name], 128, slice(0, 64)), _seq(b[name], 64, slice(0, 64))), f"{name}: Q = 2 and Q = 4 launches differ"

@pytest.mark.parametrize("B,S,L,FF", [(5, 7, 2, 384), (3, 32, 2, 2048)])
def test_every_sequence_equals_itself_launched_alone(dev, B, S, L, FF):
    """without dropout (masks are drawn by launch row) a sequence's tensors do not depend on its place in the batch; both launches share a
    sequence between the same number of workgroups (Q = 1 for FF = 384, Q = 4 for FF = 2048 at these sizes)"""
    ops, _, _, _ = _reference(Q.trunk_random, B, S, L, FF, 9, 0.0, Q.TRUNK_SITE, Q.RNG_WORD, True)
    t = _Trunk(dev, ops, 0.0)
    t.fwd()
    t.bwd()
    whole = t.results()
    for b in range(B):
        one = _Trunk(dev, dict(ops, emb=ops["emb"][b:b + 1], dpooled=ops["dpooled"][b:b + 1]), 0.0)
        one.fwd()
        one.bwd()
        for name, v in one.results().items():
            assert torch.equal(_seq(whole[name], B, slice(b, b + 1)), _seq(v, 1, slice(0, 1))), f"{name}: sequence {b} of {B} differs from itself launched alone"


@pytest.mark.parametrize("B,S", [(3, 11), (100, 19)])
def test_trunk_sequences_are_independent(dev, B, S):
    """changing sequences 1 .. leaves every output of sequence 0 bit-identical (test_padded_rows_do_not_leak for every tensor of the trunk)"""
    ops, _, _, _ = _reference(Q.trunk_random, B, S, 2, 2048, 13, Q.TRUNK_P, Q.TRUNK_SITE, Q.RNG_WORD, True)
    g = torch.Generator().manual_seed(14)
    other = dict(ops, emb=ops["emb"].clone(), dpooled=ops["dpooled"].clone())
    other["emb"][1:] = torch.randn(other["emb"][1:].shape, generator=g, dtype=torch.float64).float().double()
    other["dpooled"][1:] = torch.randn(other["dpooled"][1:].shape, generator=g, dtype=torch.float64).float().double()
    res = []
    for o in (ops, other):
        t = _Trunk(dev, o, Q.TRUNK_P)
        t.fwd()
        t.bwd()
        res.append(t.results())
    for name in res[0]:
        a, b = res[0][name], res[1][name]
        assert not torch.equal(a, b), f"{name}: the other sequences did not change at all (a broken test)"
        assert torch.equal(_seq(a, B, slice(0, 1)), _seq(b, B, slice(0, 1))), f"{name}: sequence 0 changed with the other sequences"


@pytest.mark.parametrize("B,S,L,FF", Q.TRUNK_SPLIT_CASES)
def test_split_operand_forward(dev, B, S, L, FF):
    """the forward launch with the remainder arrays forms every product from bf16 hi / lo splits of both operands: its fp32 tensors against
    the float64 forward on the weights hi + lo, the yardstick being the same forward in float32 arithmetic"""
    ops, plain, e32 = _reference(Q.trunk_split_case, B, S, L, FF)
    t = _Trunk(dev, ops, 0.0, split=True)
    t.fwd()
    got = t.results(forward_only=True)
    want, emu = dict(Q.trunk_tensors(plain)), dict(Q.trunk_tensors(e32))
    failed = []
    for name in ["x0", "pooled"] + [f"{li}.{n}" for li in range(L) for n in FP32_KEPT]:
        base = name.split(".")[-1]
        try:                                                          # every tensor's figure is printed before the first failure is raised
            compare_rows("txl_block_fwd split", f"{name} B{B} S{S} L{L} FF{FF}", Q.trunk_rows(got[name], B), Q.trunk_rows(want[name], B),
                         Q.trunk_rows(emu[name], B), SPLIT_MARGIN.get(base, DEFAULT_MARGIN))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


def test_trunk_refusals(dev):
    ops, _, _ = _reference(Q.trunk_split, 3, 5, 2, 256, 1, Q.TRUNK_SITE, Q.RNG_WORD)
    t = _Trunk(dev, ops, 0.0, split=True)
    fwd_out, all_out = t.guards(forward_only=True), t.guards()
    plain = lambda: [{k: v for k, v in r.items() if not k.endswith("_lo")} for r in t.records(False)]
    refused(lambda: t.fwd(recs=[]), REFUSED_FWD, *fwd_out)                                      # L = 0
    refused(lambda: t.bwd(recs=[]), REFUSED_BWD, *all_out)
    five = lambda backward: (t.records(backward) * 3)[:5]
    refused(lambda: t.fwd(recs=five(False)), "txl_block: at most 4 layers", *fwd_out)           # L = 5
    refused(lambda: t.bwd(recs=five(True)), "txl_block: at most 4 layers", *all_out)
    for over in (dict(S=33), dict(H=4), dict(FF=192), dict(FF=64)):
        refused(lambda: t.fwd(recs=plain(), **over), REFUSED_FWD, *fwd_out)
    chain = "hulc_txl_block: layer l+1's x is layer l's y2"
    broken = plain()
    broken[1]["x"] = t.out[0]["y1"].t                                                           # layer 1 reads something else than layer 0's output
    refused(lambda: t.fwd(recs=broken), chain, *fwd_out)
    broken_b = t.records(True)
    broken_b[1]["x"] = t.out[0]["y1"].t
    refused(lambda: t.bwd(recs=broken_b), chain, *all_out)
    together = "hulc_txl_block: pre / mean / rstd are kept together or not at all"
    lone = plain()
    del lone[0]["mean2"]
    refused(lambda: t.fwd(recs=lone), together, *fwd_out)
    need4 = "hulc_txl_block_fwd: the split-operand forward needs all four remainder arrays and the packed W1p / W2p of a layer"
    for drop in ("Wo_lo", "W1p_lo", "W2p"):
        part = t.records(False)
        for r in part:
            del r[drop]
        refused(lambda: t.fwd(recs=part), need4, *fwd_out)
    one = t.records(False)
    for k in ("Wqkv_lo", "Wo_lo", "W1p_lo", "W2p_lo"):
        del one[1][k]
    refused(lambda: t.fwd(recs=one), "hulc_txl_block_fwd: remainder arrays on every layer or on none", *fwd_out)
    null = torch.empty(0, dtype=F32, device=dev)                                                # a tensor without storage: a null pointer
    refused(lambda: t.bwd(dpooled=null), "hulc_txl_block_bwd: null pointer", *all_out)
    no_h = t.records(True)
    del no_h[0]["h"]
    refused(lambda: t.bwd(recs=no_h), REFUSED_BWD, *all_out)
