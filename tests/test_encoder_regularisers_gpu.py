"""The encoder regularisers on the GPU: dropout_vis_fc (csrc/mlp2_rows.hip, DROP instantiations), word_dropout_p (hulc_dropout_fwd) and the
l2_normalize switches (hulc_l2norm_layernorm_*_ld in csrc/pointwise.hip).

  (a) bit-exact mask pins: with W1 = 0, b1 = 1 the hidden activation hulc_mlp2_rows_bwd_drop stores IS the mask, bf16(keep-scale of element
      row * H + hidden) under a device RNG word with bits in both halves; the word-dropout launch of ones is the mirror's mask
  (b) the fused head against float64 with the replayed masks (tests/regref.py): y, dx, h, dh, both weight and both bias gradients, bf16 and
      split-operand forward, at the flat bars tests/test_mlp2_rows_gpu.py holds the same tensors to (dropout multiplies by 0 or one
      constant: no new rounding class); the GEMM-chain fallback drops the same elements; a reference whose mask is shifted by one index is
      missed by >= 3x the bar; p = 0 through the new entry points gives the old entry points' bits
  (c) hulc_l2norm_layernorm_*_ld against float64 under tests/kcheck.py (the margin class of test_reductions_gpu.py::test_layernorm_ld_forms)
  (d) the four modules with their switches on against tests/golden/regularisers/encoder_regularisers.npz, eval mode against p = 0, vis / lang masks
  (e) one Hulc2 step with all four switches on through the three loops (child processes, like the other captured-graph tests)"""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
pytestmark = pytest.mark.gpu

from hulc2_amd import functional as HF, kernels as kn, switches, synthetic as syn  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402
from oracle import counter_rng as R  # noqa: E402
from tests import errbudget, kcheck as K, regref as G  # noqa: E402
from tests.kcheck import Guarded, compare, out_flat, refused, rnd, same_bits  # noqa: E402

WORD = G.WORD
BF, F32 = torch.bfloat16, torch.float32
ON = dict(dropout_vis_fc=0.1, word_dropout_p=0.1, l2_normalize_output=True, l2_normalize_goal_embeddings=True)
MARGIN_FAST = 16.0              # kernels built on rsqrtf / sqrtf that add in another tree than torch's CPU code (tests/test_reductions_gpu.py)
EPS_LN = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    K.report("tests/test_encoder_regularisers_gpu.py")


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _bits16(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------
# (a) bit-exact mask pins
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("T", [32, 33, 96])                  # one tile, a one-row tail, three tiles
@pytest.mark.parametrize("H,OUT", [(128, 32), (512, 64), (128, 64), (512, 32)])
def test_head_backward_stores_the_mirror_mask(dev, p, T, H, OUT):
    kn.reset_step_state(dev, seed=WORD)
    seed = G.STATIC_FC_SITE
    g = torch.Generator().manual_seed(T * 1000 + H + OUT)
    x = torch.randn(T, 128, generator=g).to(dev)
    dy = torch.randn(T, OUT, generator=g).to(dev)
    W1 = torch.zeros(H, 128, dtype=BF, device=dev)
    b1 = torch.ones(H, device=dev)
    W2 = (torch.randn(OUT, H, generator=g) / H ** 0.5).to(dev).to(BF)
    h, dh, dx = Guarded(dev, T, H, BF), Guarded(dev, T, H, BF), Guarded(dev, T, 128)
    kn.mlp2_rows_bwd(x, dy, W1, b1, W1.t().contiguous(), W2.t().contiguous(), dx.t, h.t, dh.t, drop_p=p, seed=seed)
    torch.cuda.synchronize()
    for gd, nm in ((h, "h"), (dh, "dh"), (dx, "dx")):
        gd.assert_guards(nm)
    keep = G.keep_scales(seed, T, H, p, WORD)
    want = keep.float().to(BF)
    got = h.value().cpu()
    assert torch.equal(_bits16(got), _bits16(want)), int((got != want).sum())
    # dh carries mask * scale inside its gate: zero exactly where the mask is (W2^T dy is never exactly zero on these inputs)
    assert torch.equal(dh.value().cpu() == 0, keep == 0)
    assert torch.equal(dx.value(), torch.zeros_like(dx.value())), "W1 = 0: no input gradient"
    assert abs(float((keep > 0).double().mean()) - R.keep_probability(p)) < 0.03        # (4096 .. 49152 elements)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", [5 * 384, 4 * 477 + 3])        # the (5, 384) embedding; not a multiple of 4: the last draw serves three elements
def test_word_dropout_is_the_mirror_mask(dev, p, n):
    kn.reset_step_state(dev, seed=WORD)
    x = torch.ones(n, device=dev)
    y = out_flat(dev, n)
    kn.dropout_fwd(x, y.t, n, p, G.WORD_DROPOUT_SITE)
    torch.cuda.synchronize()
    y.assert_guards("y")
    want = R.dropout_scale(G.WORD_DROPOUT_SITE ^ WORD, np.arange(n, dtype=np.uint64), p)
    got = y.value().reshape(-1).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    # the helper on a (rows, 384) embedding: element index row * 384 + column
    if n == 5 * 384:
        e = torch.ones(5, 384, device=dev)
        got2 = HF.word_dropout(e, p, G.WORD_DROPOUT_SITE).cpu().numpy()
        assert np.array_equal(got2.reshape(-1).view(np.uint32), want.view(np.uint32))
        assert HF.word_dropout(e, 0.0, G.WORD_DROPOUT_SITE) is e


def test_word_dropout_refuses_what_it_cannot_run(dev):
    x, y = torch.ones(8, device=dev), out_flat(dev, 8)
    refused(lambda: kn.dropout_fwd(x, y.t, 8, 1.0, 1), "hulc_dropout_fwd: n >= 0 and drop_p in [0, 1)", y)
    refused(lambda: kn.dropout_fwd(x, y.t, -1, 0.1, 1), "hulc_dropout_fwd: n >= 0 and drop_p in [0, 1)", y)


# ------------------------------------------------------------------------------------------------
# (b) the fused head against float64 with replayed masks
# ------------------------------------------------------------------------------------------------
SEED_B = 0x5EED4001


def _head_case(T, H, OUT):
    g = torch.Generator().manual_seed(T + H + OUT)
    fc1, fc2 = torch.nn.Linear(128, H), torch.nn.Linear(H, OUT)
    with torch.no_grad():
        for q in (fc1.weight, fc1.bias, fc2.weight, fc2.bias):
            q.copy_((torch.rand(q.shape, generator=g) * 2 - 1) / (q.shape[-1] if q.dim() == 1 else q.shape[1]) ** 0.5 * (4.0 if q.dim() == 1 else 1.0))
    return fc1, fc2, torch.randn(T, 128, generator=g), torch.randn(T, OUT, generator=g)


def _head_reference(fc1, fc2, x, r, keep):
    """float64: y, dx, h, dh, dW1, db1, dW2, db2 of (y * r).sum()"""
    P = [q.detach().double().clone().requires_grad_(True) for q in (fc1.weight, fc1.bias, fc2.weight, fc2.bias)]
    xd = x.double().clone().requires_grad_(True)
    z = torch.nn.functional.linear(xd, P[0], P[1])
    z.retain_grad()                                            # the kernel's dh is the gradient of the pre-activation: the operand of dW1 = dh^T x
    h = torch.relu(z) * keep                                   # post-dropout: the operand of dW2 = dy^T h (tests/regref.py: head)
    y = torch.nn.functional.linear(h, P[2], P[3])
    (y * r.double()).sum().backward()
    return dict(y=y.detach(), dx=xd.grad, h=h.detach(), dh=z.grad, dW1=P[0].grad, db1=P[1].grad, dW2=P[2].grad, db2=P[3].grad)


def _head_gpu(dev, fc1, fc2, x, r, p, seed, kernel_tensors=True):
    """HF.mlp2_rows with dropout -> the same dictionary (h, dh from the backward launch itself, through the C ABI)"""
    for q in list(fc1.parameters()) + list(fc2.parameters()):
        q.grad = None
    xd = x.to(dev).requires_grad_(True)
    y = HF.mlp2_rows(xd, fc1.weight, fc1.bias, fc2.weight, fc2.bias, drop_p=p, seed=seed)
    (y * r.to(dev)).sum().backward()
    out = dict(y=y.detach(), dx=xd.grad, dW1=fc1.weight.grad.clone(), db1=fc1.bias.grad.clone(), dW2=fc2.weight.grad.clone(),
               db2=fc2.bias.grad.clone(), fn=type(y.grad_fn).__name__)
    if kernel_tensors:
        T, H = x.shape[0], fc1.weight.shape[0]
        W1, W2 = fc1.weight.detach().to(BF), fc2.weight.detach().to(BF)
        h, dh, dx = Guarded(dev, T, H, BF), Guarded(dev, T, H, BF), Guarded(dev, T, 128)
        kn.mlp2_rows_bwd(x.to(dev), r.to(dev), W1, fc1.bias.detach(), W1.t().contiguous(), W2.t().contiguous(), dx.t, h.t, dh.t, drop_p=p, seed=seed)
        torch.cuda.synchronize()
        for gd, nm in ((h, "h"), (dh, "dh"), (dx, "dx")):
            gd.assert_guards(nm)
        out.update(h=h.value().float(), dh=dh.value().float())
        assert torch.equal(dx.value(), out["dx"]), "the autograd node's dx is the launch's"
    torch.cuda.synchronize()
    return out


def _gemm_path_hidden(dev, fc1, fc2, x, r, p, seed):
    """the hidden activation and its pre-activation gradient as the GEMM-chain fallback forms them — the two calls functional.MLPFn makes
    for this layer: ReLU + dropout in the forward GEMM's epilogue, (g W2) * (act > 0) / (1 - p) in the data-gradient GEMM's"""
    T, H, OUT = x.shape[0], fc1.weight.shape[0], fc2.weight.shape[0]
    W1, W2T = fc1.weight.detach().to(BF), fc2.weight.detach().to(BF).t().contiguous()
    act, dz = torch.empty(T, H, device=dev), torch.empty(T, H, device=dev)
    kn.gemm(x.to(dev), W1, act, T, H, 128, 128, 128, H, bias=fc1.bias.detach(), relu=True, drop_p=p, drop_seed=seed)
    kn.gemm(r.to(dev), W2T, dz, T, H, OUT, OUT, OUT, H, mask=act, ld_mask=H, mask_scale=1.0 / (1.0 - p))
    torch.cuda.synchronize()
    return act, dz


GRADS = ("dx", "dh", "dW1", "db1", "dW2", "db2")


@pytest.mark.parametrize("T,H,OUT", [(77, 512, 64), (33, 128, 32), (96, 256, 128)])
@pytest.mark.parametrize("x3", [False, True])
def test_head_with_dropout_matches_mask_replaying_reference(dev, T, H, OUT, x3, monkeypatch):
    """Bars (relative L2), those of tests/test_mlp2_rows_gpu.py for the same tensors: y 8e-3 in bf16 and 1e-5 with the split-operand forward;
    every gradient max(1.5e-2, 1.3 x the GEMM-chain path's error against the same reference) (ReLU sign flips of pre-activations near zero
    dominate, the GEMM path sits at the same level); h — an activation rounded to bf16 on store — at y's bf16 bar 8e-3; fused against
    GEMM-chain path: y 3e-3, dx 6e-3, parameter gradients 8e-3.  Negative control: the reference with its mask shifted by one index."""
    kn.set_compute("bf16")
    if x3:
        monkeypatch.setenv("HULC_FP32_SITES", "head,encfc")
    p = 0.1
    fc1, fc2, x, r = _head_case(T, H, OUT)
    keep = G.keep_scales(SEED_B, T, H, p, WORD)
    ref = _head_reference(fc1, fc2, x, r, keep)
    shifted = _head_reference(fc1, fc2, x, r, torch.roll(keep.reshape(-1), 1).reshape(keep.shape))
    fc1, fc2 = fc1.to(dev), fc2.to(dev)
    kn.reset_step_state(dev, seed=WORD)
    import contextlib
    with (kn.site_scope("encfc") if x3 else contextlib.nullcontext()):
        got = _head_gpu(dev, fc1, fc2, x, r, p, SEED_B)
    assert got["fn"].startswith("Mlp2RowsFn")
    monkeypatch.setenv("HULC_NO_MLP2_ROWS", "1")
    gem = _head_gpu(dev, fc1, fc2, x, r, p, SEED_B, kernel_tensors=False)
    assert gem["fn"].startswith("MLPFn")
    monkeypatch.delenv("HULC_NO_MLP2_ROWS")
    gem["h"], gem["dh"] = _gemm_path_hidden(dev, fc1, fc2, x, r, p, SEED_B)
    bar = dict(y=1e-5 if x3 else 8e-3, h=8e-3)
    for k in GRADS:
        bar[k] = max(1.5e-2, 1.3 * _rel(gem[k], ref[k]))
    failures, miss = [], 0.0
    for k in ("y", "h") + GRADS:
        e = _rel(got[k], ref[k])
        print(f"[head T={T} H={H} OUT={OUT} x3={x3}] {k:4s} {e:.3e} (bar {bar[k]:.3g}; shifted mask {_rel(got[k], shifted[k]):.3e})")
        if e > errbudget.limit(k, e, bar[k]):
            failures.append(f"{k}: {e:.3e} > {bar[k]:.3g}")
        miss = max(miss, _rel(got[k], shifted[k]) / bar[k])
    assert not failures, "\n".join(failures)
    assert miss >= 3.0, miss
    if not x3:              # both HIP paths round the same operands to bf16 and drop the same elements: they differ by summation order
        assert _rel(got["y"], gem["y"]) < 3e-3 and _rel(got["dx"], gem["dx"]) < 6e-3
        for k in ("dW1", "db1", "dW2", "db2"):
            assert _rel(got[k], gem[k]) < 8e-3, (k, _rel(got[k], gem[k]))


def test_fused_head_and_gemm_fallback_drop_the_same_elements(dev):
    """b1 = 8 keeps every pre-activation positive, so a zero of the hidden activation is a dropped element and nothing else: the launch's h
    and the hidden activation of the fallback's first GEMM (ReLU + dropout epilogue, the call functional.MLPFn makes) have the same zeros,
    exactly, and they are the mirror's"""
    kn.set_compute("bf16")
    kn.reset_step_state(dev, seed=WORD)
    T, H, OUT, p = 77, 512, 64, 0.1
    fc1, fc2, x, r = _head_case(T, H, OUT)
    with torch.no_grad():
        fc1.bias.fill_(8.0)
    fc1, fc2 = fc1.to(dev), fc2.to(dev)
    got = _head_gpu(dev, fc1, fc2, x, r, p, SEED_B)
    act, _ = _gemm_path_hidden(dev, fc1, fc2, x, r, p, SEED_B)
    keep = G.keep_scales(SEED_B, T, H, p, WORD)
    assert torch.equal(act.cpu() == 0, keep == 0)
    assert torch.equal(got["h"].cpu() == 0, keep == 0)


@pytest.mark.parametrize("T,H,OUT", [(33, 128, 32), (96, 512, 64)])
def test_zero_probability_through_the_new_entry_points_is_the_old_launch(dev, T, H, OUT):
    kn.set_compute("bf16")
    fc1, fc2, x, r = _head_case(T, H, OUT)
    x, r = x.to(dev), r.to(dev)
    W1, W2 = fc1.weight.detach().to(dev).to(BF), fc2.weight.detach().to(dev).to(BF)
    b1, b2 = fc1.bias.detach().to(dev), fc2.bias.detach().to(dev)
    W1T, W2T = W1.t().contiguous(), W2.t().contiguous()
    W1lo = (fc1.weight.detach().to(dev) - W1.float()).to(BF)
    W2lo = (fc2.weight.detach().to(dev) - W2.float()).to(BF)
    for lo in ((None, None), (W1lo, W2lo)):
        y0, y1 = torch.empty(T, OUT, device=dev), Guarded(dev, T, OUT)
        kn.mlp2_rows_fwd(x, W1, b1, W2, b2, y0, *lo)
        kn._call("hulc_mlp2_rows_fwd_drop", x, W1, b1, W2, b2, lo[0], lo[1], T, 128, H, OUT, y1.t, 0.0, 12345, kn.step_state(dev))
        torch.cuda.synchronize()
        y1.assert_guards("y")
        assert torch.equal(y1.value(), y0)
    old = [torch.empty(T, 128, device=dev), torch.empty(T, H, dtype=BF, device=dev), torch.empty(T, H, dtype=BF, device=dev)]
    new = [Guarded(dev, T, 128), Guarded(dev, T, H, BF), Guarded(dev, T, H, BF)]
    kn.mlp2_rows_bwd(x, r, W1, b1, W1T, W2T, *old)
    kn._call("hulc_mlp2_rows_bwd_drop", x, r, W1, b1, W1T, W2T, T, 128, H, OUT, new[0].t, new[1].t, new[2].t, 0.0, 12345, kn.step_state(dev))
    torch.cuda.synchronize()
    for a, b, nm in zip(new, old, ("dx", "h", "dh")):
        a.assert_guards(nm)
        assert torch.equal(a.value(), b), nm


def test_head_with_dropout_is_deterministic_and_follows_the_word(dev):
    kn.set_compute("bf16")
    fc1, fc2, x, r = _head_case(96, 512, 64)
    fc1, fc2 = fc1.to(dev), fc2.to(dev)
    kn.reset_step_state(dev, seed=WORD)
    a = _head_gpu(dev, fc1, fc2, x, r, 0.1, SEED_B, kernel_tensors=False)
    b = _head_gpu(dev, fc1, fc2, x, r, 0.1, SEED_B, kernel_tensors=False)
    kn.reset_step_state(dev, seed=WORD ^ 0x100000001)
    c = _head_gpu(dev, fc1, fc2, x, r, 0.1, SEED_B, kernel_tensors=False)
    for k in ("y", "dx", "dW1", "db1", "dW2", "db2"):
        assert torch.equal(a[k], b[k]), k
        if k != "db2":                                             # (db2 is the column sum of dy: no mask reaches it)
            assert not torch.equal(a[k], c[k]), k


# ------------------------------------------------------------------------------------------------
# (c) hulc_l2norm_layernorm_fwd_ld / _bwd_ld
# ------------------------------------------------------------------------------------------------
def _l2ln_fwd(x, gamma, beta):
    n = x.norm(dim=1)
    inv = 1.0 / n.clamp_min(torch.tensor(1e-12, dtype=x.dtype))
    u = x * inv[:, None]
    mean = u.mean(dim=1)
    var = ((u - mean[:, None]) ** 2).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + EPS_LN)
    return (u - mean[:, None]) * rstd[:, None] * gamma + beta, inv, mean, rstd


def _l2ln_bwd(dy, x, inv, mean, rstd, gamma):
    u = x * inv[:, None]
    xh = (u - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    du = rstd[:, None] * (g - g.mean(dim=1, keepdim=True) - xh * (g * xh).mean(dim=1, keepdim=True))
    dx = (du - u * (u * du).sum(dim=1, keepdim=True)) * inv[:, None]
    return dx, (dy * xh).sum(dim=0), dy.sum(dim=0)


def _gen(*key):
    seed = 0
    for k in key:
        for ch in repr(k):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# R, D, ld_y, ld_dy, accumulate_params: D = 32 / 64 are the goal and camera widths, 1 and 256 the contract's ends
L2LN = [
    (5, 32, 40, 48, True),
    (64, 64, 128, 128, False),         # the cameras' halves of the 128-wide embedding
    (1, 64, 64, 64, True),             # pitch = width
    (5, 1, 2, 3, False),
    (1, 256, 300, 257, True),
    (64, 32, 33, 64, True),            # odd pitch out; 4 rows per block in the backward: 16 partial rows
    (5, 256, 256, 512, False),
]


@pytest.mark.parametrize("R_,D,ld_y,ld_dy,accumulate", L2LN)
def test_l2norm_layernorm_ld_forms(dev, R_, D, ld_y, ld_dy, accumulate):
    g = _gen("l2ln", R_, D, ld_y, ld_dy)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rnd(randn(R_, D) * (0.5 + torch.arange(R_, dtype=torch.float64)[:, None]), F32)      # rows of different norms
    gamma, beta = rnd(1.0 + 0.3 * randn(D), F32), rnd(0.2 * randn(D), F32)
    d = lambda t: t.float().to(dev)
    f = lambda t: t.float()
    y, inv, mean, rstd = Guarded(dev, R_, D, ld=ld_y), out_flat(dev, R_), out_flat(dev, R_), out_flat(dev, R_)
    args = (d(x), d(gamma), d(beta), EPS_LN, R_, D, y.t, ld_y, inv.t, mean.t, rstd.t)
    kn.l2norm_layernorm_fwd_ld(*args)
    torch.cuda.synchronize()
    for gd, nm in ((y, "y (padding columns and guard bands)"), (inv, "inv_norm"), (mean, "mean"), (rstd, "rstd")):
        gd.assert_guards(nm)
    r, f32 = _l2ln_fwd(x, gamma, beta), _l2ln_fwd(f(x), f(gamma), f(beta))
    got = (y.value(), inv.value(), mean.value(), rstd.value())
    for i, nm in enumerate(("y", "inv_norm", "mean", "rstd")):
        compare("l2norm_layernorm_fwd_ld", nm, got[i], r[i], f32[i], MARGIN_FAST)
    y.t.fill_(float("nan"))
    kn.l2norm_layernorm_fwd_ld(*args)
    torch.cuda.synchronize()
    same_bits(y.value(), got[0], "l2norm_layernorm_fwd_ld y")
    same_bits(inv.value(), got[1], "inv_norm"); same_bits(mean.value(), got[2], "mean"); same_bits(rstd.value(), got[3], "rstd")

    # backward from the float32-rounded reference statistics
    inv32, mean32, rstd32 = rnd(r[1], F32), rnd(r[2], F32), rnd(r[3], F32)
    dy = rnd(randn(R_, D), F32)
    dyg = Guarded(dev, R_, D, ld=ld_dy, init=dy)                     # a block of a wider tensor; its padding is NaN
    dg0, db0 = rnd(randn(D), F32), rnd(randn(D), F32)
    dx, dgamma, dbeta = Guarded(dev, R_, D), out_flat(dev, D), out_flat(dev, D)

    def run():
        dgamma.t.copy_(dg0.float().reshape(1, D)); dbeta.t.copy_(db0.float().reshape(1, D))
        kn.l2norm_layernorm_bwd_ld(dyg.t, ld_dy, d(x), d(inv32), d(mean32), d(rstd32), d(gamma), R_, D, dx.t, dgamma.t, dbeta.t,
                                   accumulate_params=accumulate)
        torch.cuda.synchronize()
        return dx.value(), dgamma.value(), dbeta.value()

    b1 = run()
    dx.assert_guards("dx"); dgamma.assert_guards("dgamma"); dbeta.assert_guards("dbeta"); dyg.assert_guards("dy is an input")
    rb = _l2ln_bwd(dy, x, inv32, mean32, rstd32, gamma)
    fb = _l2ln_bwd(f(dy), f(x), f(inv32), f(mean32), f(rstd32), f(gamma))
    acc = lambda t, t0, dt: t + (t0.to(dt) if accumulate else 0)
    compare("l2norm_layernorm_bwd_ld", "dx", b1[0], rb[0], fb[0], MARGIN_FAST, grad=True)
    compare("l2norm_layernorm_bwd_ld", "dgamma", b1[1], acc(rb[1], dg0, torch.float64), acc(fb[1], dg0, F32), MARGIN_FAST, grad=True)
    compare("l2norm_layernorm_bwd_ld", "dbeta", b1[2], acc(rb[2], db0, torch.float64), acc(fb[2], db0, F32), MARGIN_FAST, grad=True)
    b2 = run()
    for a, b, nm in zip(b1, b2, ("dx", "dgamma", "dbeta")):
        same_bits(b, a, "l2norm_layernorm_bwd_ld " + nm)


@pytest.mark.parametrize("D", [32, 64])
def test_l2norm_layernorm_row_of_zeros(dev, D):
    """||x|| = 0: the clamp holds, u = 0, y = beta; the gradient is that of x / 1e-12 — finite, and the float64 reference's"""
    R_ = 5
    g = _gen("l2ln0", D)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rnd(randn(R_, D), F32)
    x[2] = 0.0
    gamma, beta = rnd(1.0 + 0.3 * randn(D), F32), rnd(0.2 * randn(D), F32)
    d = lambda t: t.float().to(dev)
    y, inv, mean, rstd = Guarded(dev, R_, D), out_flat(dev, R_), out_flat(dev, R_), out_flat(dev, R_)
    kn.l2norm_layernorm_fwd_ld(d(x), d(gamma), d(beta), EPS_LN, R_, D, y.t, D, inv.t, mean.t, rstd.t)
    torch.cuda.synchronize()
    yv = y.value().cpu()
    assert torch.isfinite(yv).all() and torch.equal(yv[2], beta.float())
    assert abs(float(inv.value()[0, 2]) * 1e-12 - 1.0) < 1e-6          # 1 / max(0, 1e-12)
    dy = rnd(randn(R_, D), F32)
    dx, dgamma, dbeta = Guarded(dev, R_, D), out_flat(dev, D), out_flat(dev, D)
    kn.l2norm_layernorm_bwd_ld(d(dy), D, d(x), inv.value().reshape(-1), mean.value().reshape(-1), rstd.value().reshape(-1), d(gamma), R_, D,
                               dx.t, dgamma.t, dbeta.t)
    torch.cuda.synchronize()
    got = dx.value().cpu()
    assert torch.isfinite(got).all() and torch.isfinite(dgamma.value()).all() and torch.isfinite(dbeta.value()).all()
    stats = [t.value().reshape(-1).cpu() for t in (inv, mean, rstd)]
    rb = _l2ln_bwd(dy, x, *[s.double() for s in stats], gamma)
    fb = _l2ln_bwd(dy.float(), x.float(), *stats, gamma.float())
    compare("l2norm_layernorm_bwd_ld", "dx zero row", got[2:3], rb[0][2:3], fb[0][2:3], MARGIN_FAST, grad=True)
    live = [0, 1, 3, 4]
    compare("l2norm_layernorm_bwd_ld", "dx others", got[live], rb[0][live], fb[0][live], MARGIN_FAST, grad=True)


def test_l2norm_layernorm_refuses_what_it_cannot_run(dev):
    R_, D = 4, 257
    z = lambda *s: torch.ones(*s, device=dev)
    y, inv, mean, rstd, dx = Guarded(dev, R_, D), out_flat(dev, R_), out_flat(dev, R_), out_flat(dev, R_), Guarded(dev, R_, D)
    dg, db = out_flat(dev, D), out_flat(dev, D)
    fmsg, bmsg = "hulc_l2norm_layernorm_fwd_ld: D must be in 1..256, ld_y >= D", "hulc_l2norm_layernorm_bwd_ld: D must be in 1..256, ld_dy >= D"
    refused(lambda: kn.l2norm_layernorm_fwd_ld(z(R_, D), z(D), z(D), EPS_LN, R_, D, y.t, D, inv.t, mean.t, rstd.t), fmsg, y, inv, mean, rstd)
    refused(lambda: kn.l2norm_layernorm_bwd_ld(z(R_, D), D, z(R_, D), z(R_), z(R_), z(R_), z(D), R_, D, dx.t, dg.t, db.t), bmsg, dx, dg, db)
    D = 64                                                           # a pitch narrower than the row
    y, dx, dg, db = Guarded(dev, R_, D), Guarded(dev, R_, D), out_flat(dev, D), out_flat(dev, D)
    refused(lambda: kn.l2norm_layernorm_fwd_ld(z(R_, D), z(D), z(D), EPS_LN, R_, D, y.t, D - 1, inv.t, mean.t, rstd.t), fmsg, y, inv, mean, rstd)
    refused(lambda: kn.l2norm_layernorm_bwd_ld(z(R_, D), D - 1, z(R_, D), z(R_), z(R_), z(R_), z(D), R_, D, dx.t, dg.t, db.t), bmsg, dx, dg, db)


# ------------------------------------------------------------------------------------------------
# (d) the modules
# ------------------------------------------------------------------------------------------------
# The flat tolerances tests/test_parity_gpu.py holds the same modules' tensors to in its module tests (TOL of test_vision_encoders /
# test_goal_encoders_and_proposal: LayerNorm-ed camera embeddings `emb`, goal encoder outputs `act`, gradients `grad`).  Its BARS table
# belongs to the whole step under the selective-precision sites and has no row for a module called on its own.
from tests.test_parity_gpu import TOL, close  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(ROOT / "tests" / "golden" / "regularisers" / "encoder_regularisers.npz", allow_pickle=False))


def _model(dev, seed=G.SEED, dropout_p=0.0, **kw):
    m = instantiate(default_model_config(gripper_control=True, dropout_p=dropout_p, **kw)).to(dev)
    syn.fill_state_dict_(m.state_dict(), seed)
    m.train()
    return m


@pytest.fixture(scope="module")
def model_on(dev):
    return _model(dev, **ON)


@pytest.fixture(params=["fp32", "bf16"])
def mode(request):
    kn.set_compute(request.param)
    yield request.param
    kn.set_compute("bf16")


def _module(m, tag):
    return {"static": m.perceptual_encoder.rgb_static_encoder, "gripper": m.perceptual_encoder.rgb_gripper_encoder,
            "visual_goal": m.visual_goal, "language_goal": m.language_goal}[tag]


@pytest.mark.parametrize("tag", list(G.MODULES))
def test_modules_match_the_reference_fixture(dev, model_on, fixture, mode, tag):
    """each module in train mode with its switches on, on the fixture's inputs under the fixture's device word"""
    t = TOL[mode]
    for q in model_on.parameters():
        q.grad = None
    net = _module(model_on, tag)
    x, r = G.inputs(tag)
    x = x.float().to(dev)
    goal = tag.endswith("goal")
    if goal:
        x.requires_grad_(True)
    kn.reset_step_state(dev, seed=WORD)
    out = net(x)
    close(out, fixture[tag + ".out"], t["act"] if goal else t["emb"], "module output")
    (out * r.float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    if goal:
        close(x.grad, fixture[tag + ".gx"], t["grad"], "gx")
    named = dict(net.named_parameters())
    for name, step in G.GRAD_PARAMS[tag]:
        g = named[name].grad
        close(g[::step] if step else g, fixture[f"{tag}.g.{name}"], t["grad"], "g " + name)
    kn.check_faults(dev)


def test_eval_mode_is_the_zero_probability_model_bit_for_bit(dev, model_on):
    """nn.Dropout's rule: inactive in eval mode whatever torch.is_grad_enabled() says; the l2 flags hold in both modes"""
    kn.set_compute("bf16")
    twin = _model(dev, l2_normalize_output=True, l2_normalize_goal_embeddings=True)           # p = 0 everywhere, the same weights
    model_on.eval()
    twin.eval()
    try:
        kn.reset_step_state(dev, seed=WORD)
        for tag in G.MODULES:
            x = G.inputs(tag)[0].float().to(dev)
            a, b = _module(model_on, tag)(x), _module(twin, tag)(x)          # gradients enabled: still no dropout
            assert torch.equal(a, b), tag
            with torch.no_grad():
                assert torch.equal(_module(model_on, tag)(x), b), tag
        batch = syn.make_batch(3, 1, 4, device=dev)["vis"]
        with torch.no_grad():
            ea = model_on.perceptual_encoder(batch["rgb_obs"], batch["depth_obs"], batch["robot_obs"])
            eb = twin.perceptual_encoder(batch["rgb_obs"], batch["depth_obs"], batch["robot_obs"])
        assert torch.equal(ea, eb)
        # and train mode does differ
        model_on.train()
        x = G.inputs("language_goal")[0].float().to(dev)
        assert not torch.equal(model_on.language_goal(x), twin.language_goal(x))
    finally:
        model_on.train()
    kn.check_faults(dev)


def _embeddings_per_modality(dev, p, batched, B=2, S=4, seed=5):
    """one training step on a batch whose two modalities carry the same frames and the same language rows -> ([emb vis, emb lang], goals)"""
    kn.set_compute("bf16")
    kn.reset_step_state(dev, seed=WORD)
    m = _model(dev, seed, dropout_vis_fc=p, word_dropout_p=p)
    batch = syn.make_batch(seed, B, S, device=dev)
    batch["lang"]["rgb_obs"] = {k: v.clone() for k, v in batch["vis"]["rgb_obs"].items()}
    taps = []
    h = m.perceptual_encoder.register_forward_hook(lambda mod, i, o: taps.append(o.detach().clone()))
    m.training_step(batch, 0)
    h.remove()
    torch.cuda.synchronize()
    kn.check_faults(dev)
    if batched:
        assert len(taps) == 1
        return [taps[0][:B], taps[0][B:]]
    assert len(taps) == 2
    return taps


@pytest.mark.parametrize("arrangement", ["per_modality", "batched"])
def test_modalities_draw_different_camera_masks(dev, arrangement):
    """identical frames in both modalities: with dropout_vis_fc = 0 the two embeddings agree bit for bit, with 0.1 every frame's embedding
    differs — the stacked call's rows are distinct, the per-modality calls take per-modality sites"""
    env = dict(HULC_NO_MODALITY_BATCHING="1") if arrangement == "per_modality" else {}
    with switches.scope(HULC_NO_STEP_NODE="1", **env):
        off = _embeddings_per_modality(dev, 0.0, arrangement == "batched")
        on = _embeddings_per_modality(dev, 0.1, arrangement == "batched")
    d_off = ((off[0] - off[1]).flatten(2).norm(dim=2) / off[1].flatten(2).norm(dim=2)).cpu()
    assert float(d_off.max()) <= 1e-6, d_off
    d = ((on[0] - on[1]).flatten(2).norm(dim=2) / on[1].flatten(2).norm(dim=2)).cpu()
    print(f"[{arrangement}] per-frame distance of the modalities' embeddings with dropout_vis_fc 0.1: min {float(d.min()):.2e}")
    assert float(d.min()) > 1e-3, d
    # each camera's half differs on its own (static: columns 0..63, gripper: 64..127)
    for lo in (0, 64):
        dd = (on[0][..., lo:lo + 64] - on[1][..., lo:lo + 64]).flatten(2).norm(dim=2)
        assert float(dd.min()) > 0.0, lo


# ------------------------------------------------------------------------------------------------
# (e) one step through the three loops (child processes)
# ------------------------------------------------------------------------------------------------
def _in_child(case: str) -> None:
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), case], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, f"child `{case}` exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


def _other_eager_work(dev):
    """something that allocates, fills and launches between two steps (NOTES rule 5: a replay must not depend on what ran in between)"""
    junk = torch.zeros(1 << 16, device=dev)
    junk.fill_(3.0)
    e = HF.word_dropout(torch.ones(7, 384, device=dev), 0.3, 99)
    return float(junk.sum() + e.sum())


def _loop(dev, steps, on=True, seed=43, B=2, S=16):
    """SGD with lr = 0 (the weights never move), the trunk's dropout off and the plan sample injected: a step's loss depends on the device
    RNG word through the encoder regularisers alone.  -> (model, losses, [{name: .grad} per step])"""
    kn.set_compute("bf16")
    kn.reset_step_state(dev)
    m = _model(dev, seed, **(ON if on else {}))
    batch = syn.make_batch(seed, B, S, device=dev)
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.0)
    named = list(m.named_parameters())
    losses, grads = [], []
    for i in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = m.training_step(batch, i)
        loss.backward()
        grads.append({n: (None if p.grad is None else p.grad.detach().clone()) for n, p in named})
        opt.step()
        losses.append(float(loss))
        _other_eager_work(dev)
    torch.cuda.synchronize()
    kn.check_faults(dev)
    return m, losses, grads


def _same_grads(a, b, what):
    assert a.keys() == b.keys()
    bad = [n for n in a if (a[n] is None) != (b[n] is None) or (a[n] is not None and not torch.equal(a[n], b[n]))]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ, e.g. {bad[:3]}"


def test_step_node_with_regularisers_on(dev):
    _in_child("step_node")


def _case_step_node(dev):
    """B = 2, S = 16, all four switches on.  The plain autograd loop, the step node run eagerly and the step node's two replayed graphs see
    the same device word at every step: losses bit-identical in all three, every gradient bit-identical between the eager and the replayed
    node.  The weights never move, so consecutive replays differ through the masks alone (with the switches off all six losses are one
    number).  A switch changed on the live model makes the node capture again."""
    with switches.scope(HULC_NO_STEP_NODE="1"):
        _, lp, _ = _loop(dev, 6)
    with switches.scope(HULC_NO_STEP_NODE=None, HULC_NO_STEP_GRAPH="1"):
        me, le, ge = _loop(dev, 6)
    assert me.__dict__["_hulc_step_node"].captures == 0
    with switches.scope(HULC_NO_STEP_NODE=None, HULC_NO_STEP_GRAPH=None):
        mg, lg, gg = _loop(dev, 6)
        node = mg.__dict__["_hulc_step_node"]
        assert node.disabled is None, node.disabled
        assert (node.captures, node.eager_steps, node.replays) == (1, 2, 4), (node.captures, node.eager_steps, node.replays)
        print(f"[step node] plain {lp}\n[step node] eager {le}\n[step node] graph {lg}")
        assert lg == le and lp == le, (lp, le, lg)
        for i, (a, b) in enumerate(zip(gg, ge)):
            _same_grads(a, b, f".grad of step {i}")
        assert len(set(lg)) == 6, "every step draws fresh masks; two consecutive replays differ"
        _, loff, _ = _loop(dev, 6, on=False)
        assert len(set(loff)) == 1, loff
        # a changed switch is a new signature: two eager steps, then a second capture — never a replay of the stale graph
        mg.perceptual_encoder.rgb_static_encoder.fc1[2].p = 0.3
        batch = syn.make_batch(43, 2, 16, device=dev)
        for i in range(3):
            mg.zero_grad(set_to_none=True)
            mg.training_step(batch, 6 + i).backward()
        torch.cuda.synchronize()
        assert node.captures == 2, node.captures
    kn.check_faults(dev)


def test_arena_trainer_with_regularisers_on(dev):
    _in_child("native_loop")


def _case_native_loop(dev):
    """ArenaTrainer (SGD, lr = 0) stepping eagerly against a twin that captures and replays: losses and the whole gradient arena after every
    step, bit for bit; consecutive replays differ; eager work between replays changes nothing; a switch changed after capture() is refused"""
    from hulc2_amd.trainer import ArenaTrainer

    def run(graph):
        kn.set_compute("bf16")
        kn.reset_step_state(dev)
        m = _model(dev, 17, **ON)
        tr = ArenaTrainer(m, lr=0.0, optimizer="sgd", overlap=False)
        batch = syn.make_batch(17, 2, 16, device=dev)
        if graph:
            tr.capture(batch)
        else:
            for i in range(2):                                     # capture()'s two warm-up steps
                tr.step(batch, i)
        losses, gs = [], []
        for i in range(4):
            losses.append(float(tr.replay() if graph else tr.step(batch, 0)))
            torch.cuda.synchronize()
            gs.append(tr.flat_g.clone())
            _other_eager_work(dev)
        kn.check_faults(dev)
        return m, tr, losses, gs

    _, _, le, ge = run(False)
    m, tr, lg, gg = run(True)
    print(f"[native loop] eager losses {le}\n[native loop] replay losses {lg}")
    assert lg == le, (lg, le)
    for k, (a, b) in enumerate(zip(gg, ge)):
        n = int((a.view(torch.int32) != b.view(torch.int32)).sum())
        assert n == 0, f"gradient arena after step {k}: {n} of {a.numel()} elements differ"
    assert len(set(lg)) == 4, lg
    m.language_goal.mlp[0].p = 0.25
    with pytest.raises(RuntimeError, match=r"encoder regularisers.*capture\(\)"):
        tr.replay()
    m.language_goal.mlp[0].p = 0.1
    tr.replay()
    m.visual_goal.l2_normalize_output = False
    with pytest.raises(RuntimeError, match=r"encoder regularisers.*capture\(\)"):
        tr.replay()
    torch.cuda.synchronize()
    kn.check_faults(dev)


if __name__ == "__main__":
    assert torch.cuda.is_available()
    globals()["_case_" + sys.argv[1]](torch.device("cuda:0"))
