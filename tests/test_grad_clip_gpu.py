"""Gradient clipping on the arena: hulc_grad_norm_clip (global norm + torch's clip coefficient, one deterministic pass), the
hulc_*_step_clip entry points (the coefficient / the clamp applied in registers), ArenaTrainer(gradient_clip_val=...) eager and
captured, and the drop-in optimizers under a GradScaler.

Bars.  The norm: 1 fp32 ulp of the float64 norm of double(g) * double(s) — the sum of squares is accumulated in double (each square exact,
<= n * 2^-53 relative from the additions), sqrt and the product with s are double, and the one rounding to fp32 is half an ulp.  The
coefficient, the fused-versus-unfused steps, value clipping, pass-through, the trainer against its twin and the replays: bit for bit.  With
weight decay an FMA may pair differently, so those runs are held to tests/test_optim_rules_gpu.py's 3e-6 against torch's float64
optimizer on the clipped float64 gradients (same data, same derivation: 2x the worst fp32 restatement).  The drop-in comparison: the bars
of test_drop_in_adam_takes_the_arena_step (parameters 2e-6 of their scale + 1e-3 lr, moments 1e-6 of their largest entry)."""
import functools
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
pytestmark = pytest.mark.gpu

from hulc2_amd import kernels as kn, synthetic as syn  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402
from hulc2_amd.lib import HulcKernelError  # noqa: E402
from hulc2_amd.trainer import ArenaTrainer  # noqa: E402

LR, BAR = 2e-4, 3e-6
N = 100003                                   # n % 4 == 3: float4 body + scalar tail
N8 = 100003 // 8 * 8                         # the data test_optim_rules_gpu.py's bar was derived on


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ulp32(x: float) -> float:
    a = torch.tensor(abs(x), dtype=torch.float32)
    return float((torch.nextafter(a, torch.tensor(float("inf"))) - a).double())


@functools.lru_cache(maxsize=None)
def _data(n):
    """test_optim_rules_gpu._data: parameters ~ N(0, 1), five gradients randn * 10^(i - 2)"""
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (10.0 ** (i - 2)) for i in range(5)]
    return p0, grads


def _norm(dev, g, n, grad_scale=1.0, loss_scale=None, max_norm=1.0, out=None):
    out = torch.full((2,), -7.0, device=dev) if out is None else out
    ls = None if loss_scale is None else torch.tensor([loss_scale], dtype=torch.float32, device=dev)
    kn.grad_norm_clip(g, n, grad_scale, ls, max_norm, out)
    return out


# ---- 1 .. 4: the norm pass -----------------------------------------------------------------------------------------------------------------
def test_norm_is_exact_on_a_lattice(dev):
    """2^20 - 1 elements of +-0.5 and four of +-0.25 (index 0 and the three of the scalar tail): sum g^2 = 262144 in any order, so the norm
    is 512 bit for bit — a dropped, doubled or mis-strided element changes it.  grad_scale and loss_scale scale it exactly."""
    n = (1 << 20) + 3
    gen = torch.Generator().manual_seed(1)
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    g = sign * 0.5
    g[0], g[-3:] = 0.25 * sign[0], 0.25 * sign[-3:]
    g = g.to(dev)
    assert float(g.double().pow(2).sum()) == 262144.0
    assert float(_norm(dev, g, n)[0]) == 512.0
    assert float(_norm(dev, g, n, grad_scale=0.25)[0]) == 128.0
    assert float(_norm(dev, g, n, grad_scale=0.25, loss_scale=1024.0)[0]) == 0.125


# 33 * 2^20 + 5: the grid is capped at 2048 workgroups x 256 lanes x 4 loads of 4 elements = 8 * 2^20 elements per trip: four full trips,
# the single-load remainder loop and the scalar tail; 8 * 2^20 + 5 is exactly one trip plus both remainders
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 100003, 8 * (1 << 20) + 5, 33 * (1 << 20) + 5])
def test_norm_against_float64(dev, n):
    gen = torch.Generator(device=dev).manual_seed(n % 1000)
    worst = 0.0
    for i in (0, 2, 4) if n > (1 << 20) else range(5):
        g = torch.randn(n, generator=gen, device=dev) * (10.0 ** (i - 2))
        for gs, ls in ((1.0, None), (0.3, None), (0.25, 1024.0)):
            s = torch.tensor(gs, dtype=torch.float32)
            if ls is not None:
                s = s * torch.tensor(1.0 / float(ls), dtype=torch.float64).float()
            want = float(g.double().mul(float(s.double())).pow(2).sum().sqrt())
            got = float(_norm(dev, g, n, gs, ls)[0])
            err = abs(got - want) / _ulp32(want)
            worst = max(worst, err)
            assert err <= 1.0, f"n={n} scale 10^{i - 2} s={gs}/{ls}: norm {got!r} vs float64 {want!r}: {err:.2f} ulp"
    print(f"n={n}: worst {worst:.3f} ulp")


def test_coefficient_has_torchs_bits(dev):
    """out[1] == clamp(max_norm / (out[0] + 1e-6), max=1) as torch evaluates it on the CPU (reciprocal, multiply: three fp32 roundings), for
    norms on both sides of every threshold; NaN in, NaN out (both); inf in: norm inf, coefficient 0"""
    gen = torch.Generator().manual_seed(9)
    norms = torch.cat([torch.rand(150, generator=gen) * 2.0, torch.rand(150, generator=gen) * 12.0, torch.tensor([0.0, 0.1, 0.9, 1.0, 5.0, 1e-7, 3e4])])
    g = torch.zeros(4 * norms.numel())                             # n = 1: the norm of a one-element gradient is the element
    g[::4] = norms                                                 # (every one at a 16-byte boundary, as the pass demands of an arena)
    g = g.to(dev)
    for max_norm in (0.1, 0.9, 1.0, 5.0):
        out = torch.zeros(norms.numel(), 2, device=dev)
        for k in range(norms.numel()):
            kn.grad_norm_clip(g[4 * k:4 * k + 1], 1, 1.0, None, max_norm, out[k])
        out = out.cpu()
        assert _same(out[:, 0], norms)
        want = torch.clamp(max_norm / (out[:, 0] + 1e-6), max=1.0)
        bad = (_bits(out[:, 1]) != _bits(want)).nonzero().flatten().tolist()
        assert not bad, f"max_norm {max_norm}: {len(bad)} coefficients differ, e.g. norm {float(out[bad[0], 0])!r}: {float(out[bad[0], 1])!r} vs {float(want[bad[0]])!r}"
        assert bool((want < 1).any()) and bool((want == 1).any())
    v = torch.randn(1023, generator=gen)
    for bad_value, norm_ok, coef_ok in ((float("nan"), math.isnan, math.isnan), (float("inf"), lambda x: x == float("inf"), lambda x: x == 0.0)):
        w = v.clone()
        w[517] = bad_value
        o = _norm(dev, w.to(dev), 1023, max_norm=0.9).cpu()
        assert norm_ok(float(o[0])) and coef_ok(float(o[1])), (bad_value, o)


def test_norm_is_deterministic_and_needs_no_clean_workspace(dev):
    _, grads = _data(N)
    g = grads[3].to(dev)
    a = _norm(dev, g, N, 0.3, None, 0.9).clone()
    b = _norm(dev, g, N, 0.3, None, 0.9).clone()
    for ws in kn._grad_norm_ws.values():
        ws.fill_(float("nan"))                                     # a dirty workspace: every double stage 2 reads is rewritten by stage 1
    c = _norm(dev, g, N, 0.3, None, 0.9).clone()
    assert _same(a, b) and _same(a, c) and math.isfinite(float(a[0])) and float(a[0]) > 0


# ---- 5 .. 9: the step kernels ---------------------------------------------------------------------------------------------------------------
RULES = {"adam": dict(), "adamw": dict(), "sgd_momentum": dict(momentum=0.9), "sgd_plain": dict(momentum=0.0)}


def _steps(dev, rule, n, grads, wd=0.0, grad_scale=1.0, **clip):
    """five steps of `rule` from _data's parameters -> (p, state arenas..., bf16 shadow, remainders)"""
    p = _data(n)[0].clone().to(dev)
    k = {"adam": 2, "adamw": 2, "sgd_momentum": 1, "sgd_plain": 0}[rule]
    st = [torch.zeros(n, device=dev) for _ in range(k)]
    sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    lo = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    common = dict(grad_scale=grad_scale, lo=lo, lo_ranges=[(0, n)], **clip)
    for i, g in enumerate(grads):
        if rule == "adam":
            kn.adam_step(p, g, st[0], st[1], sh, n, LR, 0.9, 0.999, 1e-8, wd, i + 1, **common)
        elif rule == "adamw":
            kn.adamw_step(p, g, st[0], st[1], sh, n, LR, 0.9, 0.999, 1e-8, wd, i + 1, **common)
        else:
            kn.sgd_step(p, g, st[0] if st else None, sh, n, LR, RULES[rule]["momentum"], 0.0, False, wd, i + 1, **common)
    torch.cuda.synchronize()
    return (p, *st, sh, lo)


def _assert_same_run(a, b, what):
    names = ["parameters", "state 0", "state 1"][:len(a) - 2] + ["bf16 shadow", "remainders"]
    for name, x, y in zip(names, a, b):
        n = int((_bits(x) != _bits(y)).sum())
        assert n == 0, f"{what}: {n} of {x.numel()} {name} differ"


@pytest.mark.parametrize("rule", list(RULES))
def test_fused_norm_clip_equals_unfused_bitwise(dev, rule):
    """the _clip step with coefficient c on raw gradients == the old entry point fed ((g * s) * c), two torch.mul on the device"""
    s, coef = 0.3, torch.tensor([0.37], device=dev)
    grads = [g.to(dev) for g in _data(N)[1]]
    fused = _steps(dev, rule, N, grads, grad_scale=s, clip_coef_dev=coef)
    plain = _steps(dev, rule, N, [torch.mul(torch.mul(g, s), coef) for g in grads])
    _assert_same_run(fused, plain, rule)
    assert not _same(fused[0], _steps(dev, rule, N, grads, grad_scale=s)[0]), "the coefficient must have had an effect"


@pytest.mark.parametrize("rule,kw", [("adamw", dict(weight_decay=1e-2)), ("sgd_momentum", dict(momentum=0.9, weight_decay=5e-4))])
def test_norm_clip_with_weight_decay_tracks_float64(dev, rule, kw):
    s, c = 0.25, 0.37
    c32 = float(torch.tensor(c, dtype=torch.float32))
    p0, grads = _data(N8)
    ref = torch.nn.Parameter(p0.clone().double())
    opt = (torch.optim.AdamW if rule == "adamw" else torch.optim.SGD)([ref], lr=LR, **kw)
    for g in grads:
        ref.grad = g.double() * s * c32
        opt.step()
    got = _steps(dev, rule, N8, [g.to(dev) for g in grads], wd=kw["weight_decay"], grad_scale=s, clip_coef_dev=torch.tensor([c], device=dev))
    err = float((got[0].double().cpu() - ref.detach()).abs().max())
    print(f"{rule} {kw}: max err {err:.3e} (bar {BAR:.1e})")
    assert err < BAR
    assert torch.equal(got[-2], got[0].to(torch.bfloat16))


@pytest.mark.parametrize("rule", list(RULES))
def test_value_clip_equals_clamped_gradients_bitwise(dev, rule):
    s, v = 0.3, 0.05
    grads = [g.clone() for g in _data(N)[1]]
    grads[2][7], grads[2][N - 1] = float("nan"), float("nan")       # body and scalar tail: a NaN stays a NaN
    grads = [g.to(dev) for g in grads]
    fused = _steps(dev, rule, N, grads, grad_scale=s, clip_value=v)
    clamped = [torch.clamp(g * s, -v, v) for g in grads]
    assert bool(torch.isnan(clamped[2][7])) and float(clamped[4].abs().max()) == float(torch.tensor(v, dtype=torch.float32))
    plain = _steps(dev, rule, N, clamped)
    _assert_same_run(fused, plain, rule)
    assert bool(torch.isnan(fused[0][7])) and bool(torch.isnan(fused[0][N - 1])) and int(torch.isnan(fused[0]).sum()) == 2


@pytest.mark.parametrize("rule", list(RULES))
def test_clip_symbols_pass_through_without_clipping(dev, rule):
    """hulc_*_step_clip with neither a coefficient nor a value: the bits of the old entry points (weight decay on, so an FMA is in play)"""
    import ctypes as c
    from hulc2_amd import lib as L
    so = L.load()
    p0, grads = _data(N)
    grads = [g.to(dev) for g in grads]
    wd, s = 1e-2, 0.3
    want = _steps(dev, rule, N, grads, wd=wd, grad_scale=s)
    p = p0.clone().to(dev)
    k = {"adam": 2, "adamw": 2, "sgd_momentum": 1, "sgd_plain": 0}[rule]
    st = [torch.zeros(N, device=dev) for _ in range(k)]
    sh, lo = torch.zeros(N, dtype=torch.bfloat16, device=dev), torch.zeros(N, dtype=torch.bfloat16, device=dev)
    rng = (c.c_long * 2)(0, N)
    stream = torch.cuda.current_stream().cuda_stream
    for i, g in enumerate(grads):
        tail = (None, s, None, lo.data_ptr(), rng, 1, None, None, None)          # step_state .. lr_dev
        if rule == "adam":
            rc = so.hulc_adam_step_clip(p.data_ptr(), g.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), sh.data_ptr(), N, LR, 0.9, 0.999, 1e-8, wd,
                                        i + 1, *tail, None, 0.0, stream)
        elif rule == "adamw":
            rc = so.hulc_adamw_step_clip(p.data_ptr(), g.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), sh.data_ptr(), N, LR, 0.9, 0.999, 1e-8, wd,
                                         i + 1, *tail, None, 0, None, 0.0, stream)
        else:
            rc = so.hulc_sgd_step_clip(p.data_ptr(), g.data_ptr(), st[0].data_ptr() if st else None, sh.data_ptr(), N, LR, RULES[rule]["momentum"],
                                       0.0, 0, wd, i + 1, *tail, None, 0, None, 0.0, stream)
        assert rc == 0, so.hulc_last_error()
    torch.cuda.synchronize()
    _assert_same_run((p, *st, sh, lo), want, rule)


def test_clip_refusals(dev):
    """both a coefficient and a value, a negative or NaN bound: -2; arenas off 16 bytes: -4 with a coefficient as without one"""
    n = 64
    p, g, m, v = (torch.zeros(n, device=dev) for _ in range(4))
    off = torch.zeros(n + 1, device=dev)[1:]
    coef = torch.ones(1, device=dev)
    calls = {"adam": lambda p=p, **kw: kn.adam_step(p, g, m, v, None, n, LR, 0.9, 0.999, 1e-8, 0.0, 1, **kw),
             "adamw": lambda p=p, **kw: kn.adamw_step(p, g, m, v, None, n, LR, 0.9, 0.999, 1e-8, 0.0, 1, **kw),
             "sgd": lambda p=p, **kw: kn.sgd_step(p, g, m, None, n, LR, 0.9, 0.0, False, 0.0, 1, **kw)}
    for name, call in calls.items():
        with pytest.raises(HulcKernelError, match="code -2"):
            call(clip_coef_dev=coef, clip_value=0.5)
        with pytest.raises(HulcKernelError, match="code -2"):
            call(clip_value=-0.5)
        with pytest.raises(HulcKernelError, match="code -2"):
            call(clip_value=float("nan"))
        with pytest.raises(HulcKernelError, match="code -4"):
            call(p=off, clip_coef_dev=coef)
        with pytest.raises(HulcKernelError, match="code -4"):
            call(p=off)
    out = torch.zeros(2, device=dev)
    with pytest.raises(HulcKernelError, match="code -2"):
        kn.grad_norm_clip(g, n, 1.0, None, -1.0, out)
    with pytest.raises(HulcKernelError, match="code -4"):
        kn.grad_norm_clip(off, n, 1.0, None, 1.0, out)              # the arena is read in 16-byte loads
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0 and float(off.abs().max()) == 0.0, "a refused call must not have launched"


# ---- 10 .. 13: ArenaTrainer -----------------------------------------------------------------------------------------------------------------
B, S, SEED = 2, 8, 23


def _model(dev, seed, dropout_p=0.0):
    kn.set_compute("bf16")
    m = instantiate(default_model_config(gripper_control=True, dropout_p=dropout_p)).to(dev)
    syn.fill_state_dict_(m.state_dict(), seed)
    m.train()
    return m


def _trainer(dev, **kw):
    kn.reset_step_state(dev)
    m = _model(dev, SEED)
    return m, ArenaTrainer(m, overlap=False, **kw), syn.make_batch(SEED, B, S, device=dev)


def _eager(dev, steps=3, scale_arena_by=None, **kw):
    """`steps` eager steps -> (parameters after each, norms, coefficients).  scale_arena_by: per-step device coefficients the finished gradient
    arena is multiplied by in place (one torch.mul_) before optimizer_step() — the unclipped twin of a clipped trainer"""
    m, tr, batch = _trainer(dev, **kw)
    ps, norms, coefs = [], [], []
    for i in range(steps):
        if scale_arena_by is None:
            tr.step(batch, i)
        else:
            tr._forward_backward(batch, i)
            tr.buckets.finish()
            tr.flat_g.mul_(scale_arena_by[i])
            tr.optimizer_step()
        ps.append(tr.flat_p.clone())
        norms.append(tr._clip_out[0].clone())
        coefs.append(tr._clip_out[1].clone())
    torch.cuda.synchronize()
    kn.check_faults(dev)
    tr.close()
    return ps, norms, coefs


@functools.lru_cache(maxsize=None)
def _unclipped(dev):
    return _eager(dev)[0]


def test_arena_norm_is_the_norm_of_the_parameter_gradients(dev):
    """after one forward / backward the norm over the WHOLE arena equals the float64 norm over the parameters' own .grad views to 1 ulp:
    alignment padding, the fused head group's padding rows and the slices of parameters no gradient reaches are zero"""
    m, tr, batch = _trainer(dev, gradient_clip_val=1e9)
    try:
        tr._forward_backward(batch, 0)
        tr.buckets.finish()
        tr.optimizer_step()
        grads = [p.grad for p in m.parameters() if p.requires_grad]
        assert all(g is not None for g in grads) and sum(g.numel() for g in grads) < tr.total, "the arena holds padding"
        want = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))
        got = tr.last_grad_norm()
        print(f"arena norm {got!r}, per-parameter float64 {want!r}, {tr.total - sum(g.numel() for g in grads)} padding elements")
        assert want > 0 and abs(got - want) <= _ulp32(want)
        assert tr.grad_norm.shape == (1,) and tr.grad_norm.is_cuda and float(tr.grad_norm) == got
    finally:
        tr.close()
        kn.reset_step_state(dev)


def test_clipped_eager_steps_equal_an_unclipped_twin_on_scaled_gradients(dev):
    """clipping by norm, active at every step: the parameters after each of three steps are those of a trainer WITHOUT clipping whose
    gradient arena was multiplied in place by the same coefficient before optimizer_step() (Adam, no weight decay), bit for bit"""
    try:
        probe = float(_eager(dev, steps=1, gradient_clip_val=1e9)[1][0])
        clip = probe / 8.0
        ps, norms, coefs = _eager(dev, gradient_clip_val=clip)
        print(f"norm of the first step {probe!r}, gradient_clip_val {clip!r}, norms {[float(x) for x in norms]}, coefficients {[float(x) for x in coefs]}")
        assert all(0.0 < float(c) < 1.0 for c in coefs), "clipping must be active at every step"
        assert len({float(x) for x in norms}) == 3
        twin = _eager(dev, scale_arena_by=coefs)[0]
        for k, (a, b) in enumerate(zip(ps, twin)):
            n = int((_bits(a) != _bits(b)).sum())
            assert n == 0, f"after step {k}: {n} of {a.numel()} parameters differ from the twin, max |diff| {float((a - b).abs().max()):.3e}"
        assert not _same(ps[-1], _unclipped(dev)[-1]), "clipping changed nothing"
    finally:
        kn.reset_step_state(dev)


def test_inactive_clipping_changes_no_bit(dev):
    try:
        ps, norms, coefs = _eager(dev, gradient_clip_val=1e9)
        assert all(float(c) == 1.0 for c in coefs) and all(float(x) > 0 for x in norms)
        for a, b in zip(ps, _unclipped(dev)):
            assert _same(a, b)
        by_value = _eager(dev, gradient_clip_val=1e9, gradient_clip_algorithm="value")[0]
        assert _same(by_value[-1], _unclipped(dev)[-1])
        assert not _same(_eager(dev, gradient_clip_val=1e-4, gradient_clip_algorithm="value")[0][-1], _unclipped(dev)[-1])
    finally:
        kn.reset_step_state(dev)


def _in_child(case: str, *args: str) -> None:
    """run `_case_<case>(dev, *args)` of this file in a fresh interpreter: every case that captures a graph (ArenaTrainer.capture, the step
    node under Hulc2.training_step) does, so that the suite's own process makes no more captures than it did without this file (NOTES.md,
    "Round 6 ... what the fork / join took besides": graph launches of a long process depend on how many captures it has made)"""
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), case, *args], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, f"child `{case} {args}` exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


def test_replays_continue_the_clipped_eager_sequence(dev):
    _in_child("replay")


def _case_replay(dev):
    """capture() (two eager steps inside) + three replay()s == five eager steps, parameters bit for bit after every replay; the norm differs
    from replay to replay and the coefficient with it (recomputed on the device); a threshold changed after the capture is never silently
    ignored: set_gradient_clip drops the graphs, replay() raises until capture() ran again"""
    probe = float(_eager(dev, steps=1, gradient_clip_val=1e9)[1][0])
    clip = probe / 8.0
    want, wn, wc = _eager(dev, steps=5, gradient_clip_val=clip)
    m, tr, batch = _trainer(dev, gradient_clip_val=clip)
    tr.capture(batch)
    norms = []
    for k in range(3):
        tr.replay()
        torch.cuda.synchronize()
        norms.append(float(tr.grad_norm))
        assert float(tr._clip_out[1]) == float(wc[2 + k]) < 1.0 and norms[-1] == float(wn[2 + k])
        n = int((_bits(tr.flat_p) != _bits(want[2 + k])).sum())
        assert n == 0, f"after replay {k}: {n} of {tr.total} parameters differ from the eager sequence"
    print(f"[replay] gradient_clip_val {clip!r}, norms of the replays {norms}")
    assert len(set(norms)) == 3, "the norm is recomputed by every replay"
    tr.set_gradient_clip(clip)                                      # the same threshold: nothing to drop
    assert tr.graph_opt is not None
    tr.set_gradient_clip(clip / 2)
    assert tr.graph_fb is None and tr.graph_opt is None
    with pytest.raises(RuntimeError, match="no captured graphs"):
        tr.replay()
    before = tr.flat_p.clone()
    tr.step(batch, 0)                                              # eager steps go on, under the new threshold
    torch.cuda.synchronize()
    assert abs(float(tr._clip_out[1]) * (tr.last_grad_norm() + 1e-6) - clip / 2) <= 1e-6 * clip and not _same(before, tr.flat_p)
    kn.check_faults(dev)
    tr.close()


# ---- 14: the drop-in optimizer under fp16 autocast + GradScaler ---------------------------------------------------------------------------------
def test_drop_in_adam_clips_inside_the_fused_step(dev):
    _in_child("drop_in")                                           # (the step node captures graphs: see _in_child)


def _case_drop_in(dev):
    """hulc2_amd.optim.Adam(max_grad_norm=...) in the reference's loop against torch.optim.Adam + scaler.unscale_ + clip_grad_norm_ on the
    same (scaled) gradients: the bars of test_drop_in_adam_takes_the_arena_step; every step fused, `.grad` untouched by step(), a step
    with an injected inf skipped without moving the step count"""
    from hulc2_amd.optim import Adam

    kn.set_compute("bf16")
    try:
        lr, max_norm = 2e-4, 1.0
        batch = syn.make_batch(5, 2, 8, device=dev)
        for db in batch.values():
            db.pop("plan_idx", None)
        m = instantiate(default_model_config(gripper_control=True, dropout_p=0.0)).to(dev)
        syn.fill_state_dict_(m.state_dict(), 11)
        m.train()
        opt = Adam(m.parameters(), lr=lr, max_grad_norm=max_norm)
        clones = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
        ref = torch.optim.Adam(clones, lr=lr)
        kn.reset_step_state(dev)
        scaler, ref_scaler = torch.amp.GradScaler("cuda", init_scale=1024.0), torch.amp.GradScaler("cuda", init_scale=1024.0)
        ref_scaler.scale(torch.zeros(1, device=dev))                # (a scaler makes its scale tensor at the first scale())
        for i in range(4):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16):
                loss = m.training_step(batch, i)
            scaler.scale(loss).backward()
            if i == 3:
                next(p for p in m.parameters() if p.grad is not None).grad.view(-1)[0] = float("inf")
                frozen = [p.detach().clone() for p in m.parameters()]
            if i == 0:                                               # a threshold a quarter of the first step's norm: clipping is active
                first = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad / 1024.0) for p in m.parameters() if p.grad is not None]))
                max_norm = float(first) / 4.0
                opt.set_grad_clip(max_norm=max_norm)
            for c, p in zip(clones, m.parameters()):
                c.grad = None if p.grad is None else p.grad.detach().clone()
            kept = [None if p.grad is None else p.grad.detach().clone() for p in m.parameters()]
            scaler.step(opt)                                         # the drop-in is handed grad_scale / found_inf: unscale, norm, clip in its kernels
            scaler.update()
            ref_scaler.unscale_(ref)
            norm = torch.nn.utils.clip_grad_norm_(clones, max_norm)
            ref_scaler.step(ref)
            ref_scaler.update()
            for k, p in zip(kept, m.parameters()):
                assert (k is None and p.grad is None) or _same(k, p.grad), ".grad must be left as backward wrote it"
            if i < 3:
                got = float(opt._clip_out[0])
                print(f"step {i}: gradient norm {got!r} (torch {float(norm)!r}), coefficient {float(opt._clip_out[1])!r}")
                assert float(norm) > max_norm and float(opt._clip_out[1]) < 1.0, "clipping must be active"
                assert abs(got - float(norm)) <= 1e-5 * float(norm)  # (torch: fp32 per-tensor norms and a norm of norms)
        torch.cuda.synchronize()
        kn.check_faults(dev)
        assert opt.fused_launches == 4, "every step, the skipped one included, is the fused launch"
        for (n, p), c, f in zip(m.named_parameters(), clones, frozen):
            assert _same(p.detach(), f), f"{n}: changed by a step the scaler found an inf in"
            assert float((p.detach() - c.detach()).abs().max()) <= 2e-6 * max(float(c.detach().abs().max()), 1.0) + 1e-3 * lr, n
        sa, sb = ref.state_dict(), opt.state_dict()
        assert sa["state"].keys() == sb["state"].keys()
        assert sb["param_groups"][0]["max_grad_norm"] == max_norm
        for k in sa["state"]:
            assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"]) == 3.0, "the skipped step does not count"
            for key in ("exp_avg", "exp_avg_sq"):
                x, y = sa["state"][k][key], sb["state"][k][key]
                assert float((x - y).abs().max()) <= 1e-6 * max(float(x.abs().max()), 1e-30), (k, key)
    finally:
        kn.reset_step_state(dev)


if __name__ == "__main__":
    assert torch.cuda.is_available()
    globals()["_case_" + sys.argv[1]](torch.device("cuda:0"), *sys.argv[2:])
