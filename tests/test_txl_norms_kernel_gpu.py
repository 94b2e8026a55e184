"""Kernel-level tests of the whole-trunk launches with the two optional LayerNorms (csrc/txl_block_norms.hip): kn.txl_block_desc +
kn.txl_block_norms + kn.txl_block_norms_fwd / _bwd called directly, every kept tensor and every backward output — the trunk's and the new
stages' — checked on its own against tests/normref.py, in the pattern of tests/test_txl_block_kernel_gpu.py (whose operand holder this
file extends):

  * random cases {LN_pos only, LN_enc only, both} x p in {0, 0.1} at S = 1, at Q = 1 with dead lanes, at Q = 2 and at Q = 4;
  * exact cases: gamma = 0 turns a LayerNorm into the constant beta, which pins where each stage sits (dropout BEHIND LN_pos with the plain
    launch's mask; LN_enc ahead of the mean) bit for bit;
  * bit equality: the tensors ahead of the first exchange between Q = 4, 2 and 1 launches of the same operands; every sequence of a batch
    against itself launched alone; both stages off through the new entry points against hulc_txl_block_fwd / _bwd;
  * the refusals of include/hulc2_amd.h, with untouched outputs.
Every launch is followed by kn.check_faults."""
import time

import pytest
import torch

from tests import kcheck as K
from tests import normref as N
from tests import seqref as Q
from tests import test_txl_block_kernel_gpu as T
from tests.kcheck import Guarded, compare_rows, refused, same_bits

pytestmark = pytest.mark.gpu

# margin * max(e_ref, 2^-23) per sequence, e_ref = normref's float32 emulation (the bf16 rounding points of the layers; the new stages are
# float32 arithmetic on both sides).  Default 2; an entry here is an exception with its measured ratio, shape and cause.
MARGIN = {}
DEFAULT_MARGIN = 2.0

E, NH, F32 = Q.E, Q.NH, torch.float32
EPS = 1e-5
CASES = [(1, 1, 1, 128), (3, 7, 1, 128), (8, 32, 2, 256), (16, 5, 2, 512)]          # S = 1; Q = 1 with dead lanes; Q = 2; Q = 4
STAGES = {"pos": (True, False), "enc": (False, True), "both": (True, True)}
NEEDS = "needs d_model 128, 8 heads, 1 <= S <= 32, 1 <= L <= 4, FF a multiple of 128 and non-null operands"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    K.report("tests/test_txl_norms_kernel_gpu.py")
    print(f"[kcheck-time] tests/test_txl_norms_kernel_gpu.py {time.time() - t0:.1f} s")


class _NormTrunk(T._Trunk):
    """the trunk's operands + the LayerNorm parameters that are on (ops["pos_norm"] / ops["enc_norm"]) and guarded outputs of both stages"""

    def __init__(self, dev, ops, p, **kw):
        super().__init__(dev, ops, p, **kw)
        self.par = {}
        for stage in ("pos", "enc"):
            if ops.get(stage + "_norm") is not None:
                g, b = ops[stage + "_norm"]
                self.par[stage + "_g"], self.par[stage + "_b"] = self._copy(g, F32, stage + "_g"), self._copy(b, F32, stage + "_b")
        G = lambda rows, cols: Guarded(dev, rows, cols, F32)
        self.nout = dict(pre0=G(self.T, E), mean0=G(1, self.T), rstd0=G(1, self.T), lnp0=G(2 * self.B, E), meanF=G(1, self.T), rstdF=G(1, self.T),
                         lnpF=G(2 * self.B, E))

    def on(self):
        return [n for n in N.NORM_KEPT + N.NORM_BWD if (n.endswith("0") and "pos_g" in self.par) or (n.endswith("F") and "enc_g" in self.par)]

    def norms(self, backward, keep=True, **over):
        from hulc2_amd import kernels as kn

        t = dict(self.par)
        for n in self.on():
            if (n in N.NORM_BWD and backward) or (n in N.NORM_KEPT and (keep or backward)):
                t[n] = self.nout[n].t
        t.update(over)
        return kn.txl_block_norms(**t)

    def fwd(self, recs=None, norms=None, share=None, B=None, S=None, H=NH, FF=None):
        from hulc2_amd import kernels as kn

        B, S, FF = B or self.B, S or self.S, FF or self.FF
        recs = self.records(False) if recs is None else recs
        d = kn.txl_block_desc(self.emb, self.pos, self.pos_ids, B, S, H, FF, self.p, self.site, EPS, recs, pooled=self.pooled.t, share=share)
        kn.txl_block_norms_fwd(d, self.norms(False) if norms is None else norms, B, S, H, E, FF, len(recs))
        torch.cuda.synchronize()
        kn.check_faults(self.dev)

    def bwd(self, recs=None, norms=None, share=None, **over):
        from hulc2_amd import kernels as kn

        recs = self.records(True) if recs is None else recs
        d = kn.txl_block_desc(self.emb, self.pos, self.pos_ids, self.B, self.S, NH, self.FF, self.p, self.site, EPS, recs,
                              dpooled=over.get("dpooled", self.dpooled), demb=over.get("demb", self.demb.t), share=share)
        kn.txl_block_norms_bwd(d, self.norms(True) if norms is None else norms, self.B, self.S, NH, E, self.FF, len(recs))
        torch.cuda.synchronize()
        kn.check_faults(self.dev)

    def guards(self, forward_only=False):
        return super().guards(forward_only) + list(self.nout.values())

    def results(self, forward_only=False):
        r = super().results(forward_only)                           # (asserts every guard band, the new stages' included)
        for n in self.on():
            if n in N.NORM_KEPT or not forward_only:
                r[n] = self.nout[n].value()
        for n in set(self.nout) - set(self.on()):
            self.nout[n].assert_untouched(f"{n} of a stage that is off")
        return r


def _ops(B, S, L, FF, seed, p, pos_on, enc_on, reference=True):
    if reference:
        return T._reference(N.trunk_random, B, S, L, FF, seed, p, Q.TRUNK_SITE, Q.RNG_WORD, pos_on, enc_on)
    ops, _, _, _ = Q.trunk_random(B, S, L, FF, seed, p, Q.TRUNK_SITE, Q.RNG_WORD, ops_only=True)
    ops["pos_norm"] = N.random_norm(seed + 1000) if pos_on else None
    ops["enc_norm"] = N.random_norm(seed + 2000) if enc_on else None
    return ops


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("stages", list(STAGES))
@pytest.mark.parametrize("B,S,L,FF", CASES)
def test_norms_random_against_float64(dev, B, S, L, FF, stages, p):
    pos_on, enc_on = STAGES[stages]
    ops, plain, e32 = _ops(B, S, L, FF, 31 * B + S, p, pos_on, enc_on)
    who = f"B{B} S{S} L{L} FF{FF} {stages} p{p}"
    t = _NormTrunk(dev, ops, p)
    t.fwd()
    t.bwd()
    got = t.results()
    want, emu = dict(N.trunk_tensors(plain)), dict(N.trunk_tensors(e32))
    assert set(got) == set(want)
    assert ("pre0" in got) == pos_on and ("lnpF" in got) == enc_on
    failed = []
    for name in want:
        base = name.split(".")[-1]
        kernel = "txl_block_norms_fwd" if base in Q.TRUNK_KEPT + N.NORM_KEPT + ("x0", "pooled") else "txl_block_norms_bwd"
        try:                                                          # every tensor's figure is printed before the first failure is raised
            compare_rows(kernel, f"{name} {who}", Q.trunk_rows(got[name], B), Q.trunk_rows(want[name], B), Q.trunk_rows(emu[name], B),
                         MARGIN.get(base, DEFAULT_MARGIN))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    t.fwd()
    t.bwd()
    for name, v in t.results().items():
        same_bits(got[name], v, f"{who} {name}")
    # inference keeps nothing of the new stages either and pools the same rows
    ti = _NormTrunk(dev, ops, p)
    ti.fwd(recs=ti.records(False, keep=False), norms=ti.norms(False, keep=False))
    for n in ti.nout:
        ti.nout[n].assert_untouched(f"{who} {n} (inference)")
    same_bits(got["pooled"], ti.pooled.value(), f"{who} pooled (nothing kept)")


@pytest.mark.parametrize("B,S,L,FF", [(3, 8, 1, 128), (8, 32, 2, 256)])
def test_norms_exact_pieces(dev, B, S, L, FF):
    """gamma = 0: LN_pos(.) = pos_b whatever its input, so layers[0].x must be pos_b * keep with the PLAIN launch's keep (dropout behind the
    LayerNorm, pos_add_seq's stream and element index); LN_enc(.) = enc_b, so pooled = enc_b, and the dbeta half of lnpF is S times
    dpooled / S = dpooled bit for bit at S a power of two"""
    ops = _ops(B, S, L, FF, 5, 0.5, False, False, reference=False)
    zero = torch.zeros(E, dtype=torch.float64)
    pos_b = (torch.arange(E) % 7 - 3).double()
    enc_b = (torch.arange(E) % 5 - 2).double()
    ops.update(pos_norm=(zero, pos_b), enc_norm=(zero, enc_b), dpooled=Q.bf(ops["dpooled"]))   # (8 mantissa bits: every partial sum k * dpooled / S is exact)
    keep = Q.trunk_keep(0.5, Q.TRUNK_SITE, Q.RNG_WORD, B, S, FF, L)
    t = _NormTrunk(dev, ops, 0.5)
    t.fwd()
    t.bwd()
    got = t.results()
    T._exact(got["x0"], pos_b[None] * keep["pos"], f"B {B} S {S} layers[0].x = pos_b * keep")
    T._exact(got["pooled"], enc_b[None].expand(B, E), f"B {B} S {S} pooled = enc_b")
    T._exact(got["lnpF"].reshape(B, 2, E)[:, 1], ops["dpooled"], f"B {B} S {S} dbeta partials of LN_enc = dpooled")
    plain = T._Trunk(dev, dict(ops, emb=torch.zeros_like(ops["emb"]), pos=torch.ones_like(ops["pos"])), 0.5)
    plain.fwd()
    mask = plain.results(forward_only=True)["x0"]                    # 1 * keep: the plain launch's mask itself
    assert torch.equal(got["x0"], mask * pos_b.float().to(mask.device)[None]), "the launch with LN_pos drops other elements than the plain launch"
    for v in got.values():
        assert torch.isfinite(v.float()).all()


def test_norm_stages_do_not_depend_on_the_share_factor(dev):
    """pre0 / mean0 / rstd0 and layers[0].x lie ahead of the first exchange: launches of the same 40 sequences at Q = 4 (the whole device:
    40 x 4 workgroups), Q = 2 (half of it) and Q = 1 (a quarter) store the same bits, and every member of a shared sequence stored them"""
    B, S, L, FF = 40, 5, 1, 512
    ops = _ops(B, S, L, FF, 17, Q.TRUNK_P, True, True, reference=False)
    res = []
    for share in (1, 2, 4):
        t = _NormTrunk(dev, ops, Q.TRUNK_P)
        t.fwd(share=share)
        t.bwd(share=share)
        res.append(t.results())
    for name in ("pre0", "mean0", "rstd0", "x0", "0.y1", "0.pre1", "0.mean1", "0.rstd1", "0.ctx"):
        for other, q in ((res[1], 2), (res[2], 1)):
            assert torch.equal(res[0][name], other[name]), f"{name}: Q = 4 and Q = {q} launches differ"


@pytest.mark.parametrize("B,S,L,FF", [(5, 7, 2, 384), (3, 32, 2, 2048)])
def test_every_sequence_equals_itself_launched_alone(dev, B, S, L, FF):
    ops = _ops(B, S, L, FF, 9, 0.0, True, True, reference=False)
    t = _NormTrunk(dev, ops, 0.0)
    t.fwd()
    t.bwd()
    whole = t.results()
    for b in range(B):
        one = _NormTrunk(dev, dict(ops, emb=ops["emb"][b:b + 1], dpooled=ops["dpooled"][b:b + 1]), 0.0)
        one.fwd()
        one.bwd()
        for name, v in one.results().items():
            assert torch.equal(T._seq(whole[name], B, slice(b, b + 1)), T._seq(v, 1, slice(0, 1))), f"{name}: sequence {b} of {B} differs from itself launched alone"


@pytest.mark.parametrize("B,S,L,FF", [(3, 7, 1, 128), (8, 32, 2, 256)])
def test_both_stages_off_is_the_plain_launch(dev, B, S, L, FF):
    ops = _ops(B, S, L, FF, 23, Q.TRUNK_P, False, False, reference=False)
    a, b = T._Trunk(dev, ops, Q.TRUNK_P), _NormTrunk(dev, ops, Q.TRUNK_P)
    for t in (a, b):
        t.fwd()
        t.bwd()
    ra, rb = a.results(), b.results()                                # (rb: also asserts that nothing of a switched-off stage was written)
    assert set(ra) == set(rb)
    for name in ra:
        assert torch.equal(ra[name], rb[name]), f"{name}: hulc_txl_block_norms_* with both stages off differs from hulc_txl_block_*"


def test_norms_refusals(dev):
    ops = _ops(3, 5, 2, 256, 1, 0.0, True, True, reference=False)
    t = _NormTrunk(dev, ops, 0.0)
    fwd_out, all_out = t.guards(forward_only=True), t.guards()
    null = torch.empty(0, dtype=F32, device=dev)                     # a tensor without storage: a null pointer
    pair = "hulc_txl_block_norms: gamma and beta of a stage come together"
    for k in ("pos_b", "pos_g", "enc_b", "enc_g"):
        refused(lambda: t.fwd(norms=t.norms(False, **{k: null})), pair, *fwd_out)
        refused(lambda: t.bwd(norms=t.norms(True, **{k: null})), pair, *all_out)
    refused(lambda: t.fwd(norms=t.norms(False, mean0=null)), "hulc_txl_block_norms: pre0 / mean0 / rstd0 are kept together or not at all", *fwd_out)
    refused(lambda: t.fwd(norms=t.norms(False, rstdF=null)), "hulc_txl_block_norms: meanF / rstdF are kept together or not at all", *fwd_out)
    need = "hulc_txl_block_norms_bwd: an enabled stage needs its kept statistics and its partial buffer"
    for k in ("lnp0", "lnpF"):
        refused(lambda: t.bwd(norms=t.norms(True, **{k: null})), need, *all_out)
    refused(lambda: t.bwd(norms=t.norms(True, pre0=null, mean0=null, rstd0=null)), need, *all_out)
    refused(lambda: t.bwd(norms=t.norms(True, meanF=null, rstdF=null)), need, *all_out)
    # everything the plain launches refuse, under the new names
    for over in (dict(S=33), dict(H=4), dict(FF=192)):
        refused(lambda: t.fwd(**over), "hulc_txl_block_norms_fwd: " + NEEDS, *fwd_out)
    refused(lambda: t.fwd(recs=[]), "hulc_txl_block_norms_fwd: " + NEEDS, *fwd_out)
    refused(lambda: t.bwd(recs=[]), "hulc_txl_block_norms_bwd: " + NEEDS, *all_out)
    refused(lambda: t.bwd(dpooled=null), "hulc_txl_block_norms_bwd: null pointer", *all_out)
    no_h = t.records(True)
    del no_h[0]["h"]
    refused(lambda: t.bwd(recs=no_h), "hulc_txl_block_norms_bwd: " + NEEDS, *all_out)
    broken = t.records(False)
    broken[1]["x"] = t.out[0]["y1"].t
    refused(lambda: t.fwd(recs=broken), "hulc_txl_block: layer l+1's x is layer l's y2", *fwd_out)
