"""The CPU references of tests/mlpref.py checked on the CPU: the lattice builders' exactness claims (every exchanged activation equals its
bf16 rounding, float32 accumulation in two different orders gives the float64 bits), the permutation chains' coverage of every
(wave, k-step, 8-group) slot, the coverage of every k-split instance by the listed shapes, and the yardsticks of the random cases of
tests/test_mlp_chain_kernel_gpu.py and tests/test_mlp2_rows_kernel_gpu.py (printed per case)."""
import pytest
import torch

from tests import mlpref as R
from tests.kcheck import EPS32, row_errors

MARGIN = 2.0
ALL_SHAPES = R.CHAIN_SHAPES + R.CHAIN_SHAPES_4096


@pytest.fixture(autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(8, n))
    yield
    torch.set_num_threads(n)


def test_listed_shapes_run_every_k_split_as_first_and_as_later_layer():
    seen = R.ksw_coverage(ALL_SHAPES)
    assert set(seen) == set(R.KSW_SET), seen
    for ksw, (first, later) in seen.items():
        assert first and later, f"KSW {ksw}: runs as layer 0: {first}, as a later layer: {later}"
    for K0, widths in ALL_SHAPES:                                     # K no multiple of 32 or 128 where the k-split allows a choice
        assert K0 % 128 != 0 or K0 == 4096


@pytest.mark.parametrize("K0,widths", ALL_SHAPES)
def test_permutation_chain_covers_every_slot_and_relocates(K0, widths):
    for M in ((1, 64) if max(widths) > 1024 or K0 > 1024 else R.CHAIN_M):
        case = R.perm_chain(M, K0, widths, seed=M, amp=R.perm_amp(K0, widths))      # (asserts coverage and exactness)
        K = K0
        for l, lay in enumerate(case["layers"]):
            W = lay["W"]
            slots = {R.k_slot(int(c), R.ksw_of(K)) for c in W.nonzero()[:, 1]}
            assert len(slots) == K // 8 and set(W.unique().tolist()) == {0.0, 1.0}
            K = W.shape[0]
        outs = R.chain_free(case)
        if all(int((lay["W"] != 0).sum(1).max()) == 1 for lay in case["layers"]):
            assert set(outs[-1].unique().tolist()) <= set(case["x0"].unique().tolist()), "a one-entry-per-row chain relocates input values"
        assert outs[-1].abs().max() > 0


@pytest.mark.parametrize("K0,widths", ALL_SHAPES)
def test_dense_lattices_are_exact(K0, widths):
    deep = len(widths) > 3
    kw = R.DEEP_KW if deep else {}
    for M in ((5, 64) if max(widths) > 1024 or K0 > 1024 else R.CHAIN_M):
        for variant in (dict(), dict(bias=False, relu=False), dict(relu=True)):
            case = R.dense_chain(M, K0, widths, seed=M + len(variant), **kw, **variant)          # (asserts its claims)
            outs = R.chain_free(case)
            assert all(o.abs().max() > 0 for o in outs)
        if len(widths) <= 3:
            R.dense_chain(M, K0, widths, seed=M + 7, masks=True, **R.MASK_KW)
        if len(widths) <= 2 and M <= 32 and max(widths) <= 2048 and K0 <= 2048:
            c3 = R.dense_chain(M, K0, widths, seed=M + 9, x3=True)
            assert (R.split(c3["x0"])[1] != 0).any(), "the split-operand lattice has no lo part"
        if len(widths) > 1:
            R.dense_chain(M, K0, widths, seed=M + 11, last_random=True, **kw)


@pytest.mark.parametrize("K0,widths", ALL_SHAPES)
def test_chain_yardsticks(K0, widths):
    """teacher-forced per layer (on the CPU the float32 emulation's own outputs stand in for the GPU's): the float64-accumulating emulation
    IS the reference, so the rounding points alone score 0; e_ref is printed per layer"""
    for M, masks, x3 in ((17, False, False), (64, False, False), (5, True, False), (17, False, True)):
        if x3 and (K0 > 2048 or max(widths) > 2048):
            continue
        case = R.random_chain(M, K0, widths, seed=K0 + M, masks=masks, x3=x3)
        fed = R.chain_free(case, R.chain_layer_emu32)
        ref = R.chain_forced(case, fed)
        e32 = R.chain_forced(case, fed, R.chain_layer_emu32)
        e64 = R.chain_forced(case, fed, R.chain_layer_ref)
        for l, (a, b, c) in enumerate(zip(ref, e32, e64)):
            live = a.norm(dim=1) > 0
            e_ref = row_errors(b[live], a[live]).max().item() if live.any() else 0.0
            assert torch.equal(a, c), "the float64-accumulating emulation is the reference"
            print(f"[mlpref] chain K0 {K0} widths {widths} M {M} masks {masks} x3 {x3} layer {l}: e_ref {e_ref:.3e} "
                  f"(floor 2^-23 = {EPS32:.3e}); float64-accumulating emulation 0.000 x")
            assert e_ref < 1e-5, f"layer {l}: yardstick {e_ref}"


@pytest.mark.parametrize("H", R.MLP2_H)
@pytest.mark.parametrize("OUT", R.MLP2_OUT)
def test_mlp2_lattices_are_exact_and_yardsticks(H, OUT):
    for T in R.MLP2_T:
        for x3 in (False, True):
            ops, want = R.mlp2_lattice(T, H, OUT, R.mlp2_seed(T, H, OUT, x3), x3)                 # (asserts its claims)
            assert want[1].max() > 256 or x3 or T < 31, "no hidden value above 256: the bf16 rounding of h is not exercised"
            assert all(float(t.abs().max()) > 0 for t in want)
            ops, ref, e32 = R.mlp2_random(T, H, OUT, R.mlp2_seed(T, H, OUT, x3), x3)
            for name, a, b in zip(("y", "h", "dh", "dx"), ref, e32):
                live = a.norm(dim=1) > 0
                e_ref = row_errors(b[live], a[live]).max().item()
                print(f"[mlpref] mlp2 T {T} H {H} OUT {OUT} x3 {x3} {name}: e_ref {e_ref:.3e}")
                assert e_ref < (1e-5 if name in ("y", "h") else 2e-2), f"{name}: yardstick {e_ref}"


def test_kernel_order_emulation():
    """chain_layer_tree32 (the kernel's 4-wave order, 32 or 8 k-terms per rounding) gives the lattices' exact bits and, on the random
    split-operand case that scored 2.78 x three separate float32 GEMMs on the GPU, an error inside the margin of the one-accumulator
    yardstick (printed)"""
    for case in (R.dense_chain(17, 264, (384, 32), seed=3), R.dense_chain(17, 40, (48, 16), seed=4, x3=True),
                 R.perm_chain(33, 136, (256, 144, 16), seed=5)):
        a = case["x0"]
        for lay in case["layers"]:
            want = R.chain_layer_ref(a, **R._layer_args(case, lay))
            for group in (32, 8):
                assert torch.equal(R.chain_layer_tree32(a, **R._layer_args(case, lay), group=group), want)
            a = want
    case = R.random_chain(17, 1000, (2048, 16), seed=1017, x3=True)
    a = R.chain_free(case, R.chain_layer_emu32)[0]
    args = R._layer_args(case, case["layers"][1])
    ref, e32 = R.chain_layer_ref(a, **args), R.chain_layer_emu32(a, **args)
    e_ref = row_errors(e32, ref).max().item()
    for group in (32, 8):
        e = row_errors(R.chain_layer_tree32(a, **args, group=group), ref).max().item()
        print(f"[mlpref] x3 K 2048: kernel-order emulation, {group} k-terms per rounding: {e:.3e} = {e / e_ref:.2f} x e_ref {e_ref:.3e}")
        assert e <= MARGIN * e_ref


def test_layer_reference_matches_torch_linear():
    """the float64 layer on bf16-exact operands is torch's own Linear (+ ReLU), and the mask wins over relu"""
    g = torch.Generator().manual_seed(3)
    a = R.bf(torch.randn(7, 40, generator=g, dtype=torch.float64))
    W = R.bf(torch.randn(16, 40, generator=g, dtype=torch.float64))
    b = torch.randn(16, generator=g, dtype=torch.float64).float().double()
    want = torch.nn.functional.linear(a, W, b)
    assert torch.allclose(R.chain_layer_ref(a, W, b), want, rtol=0, atol=1e-12)
    assert torch.allclose(R.chain_layer_ref(a, W, b, relu=True), want.clamp_min(0), rtol=0, atol=1e-12)
    mask = torch.randn(7, 16, generator=g, dtype=torch.float64)
    got = R.chain_layer_ref(a, W, b, relu=True, mask=mask, mask_scale=1.25)
    assert torch.allclose(got, torch.where(mask > 0, want * 1.25, torch.zeros(())), rtol=0, atol=1e-12) and (got < 0).any()
    # split operands: hi + lo of an fp32 input, three products, no lo x lo term
    v = torch.randn(7, 40, generator=g, dtype=torch.float64).float().double()
    w = torch.randn(16, 40, generator=g, dtype=torch.float64).float().double()
    (vh, vl), (wh, wl) = R.split(v), R.split(w)
    got = R.chain_layer_ref(v, wh, None, x3=True, W_lo=wl)
    assert torch.allclose(got, vh @ wh.t() + vl @ wh.t() + vh @ wl.t(), rtol=0, atol=1e-12)
    assert ((got - v @ w.t()).abs().max() < 2e-3) and ((R.chain_layer_ref(v, wh) - v @ w.t()).abs().max() > 1e-2)
