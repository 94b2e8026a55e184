"""Gradient accumulation in the native loop (ArenaTrainer(accumulate_grad_batches=k)), on the GPU:
  * hulc_grad_accumulate against the same fp32 expression evaluated by torch on the CPU, bit for bit (NaNs by position), and its refusals
  * an eager window: the optimizer sees ((g_1 + g_2) + g_3) * fp32(1 / 3) of a twin's gradients, nothing moves before the window closes
  * k = 1 is today's trainer; the lr schedule, clipping and the step count go by windows
  * graph mode: one forward/backward graph per micro-batch, the optimizer graph per window, equal to the eager loop
  * a checkpoint taken inside a window resumes it; one exchange per window on the RCCL path

The cases that capture graphs run in a child process each (`_in_child`), exactly as tests/test_lr_schedule_gpu.py does and for its stated
reason: graph launches of this HIP runtime have died depending on how many captures the process had made before, and the tests that follow
in the suite's process should see the same number of earlier captures with or without this file."""
import ctypes
import functools
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
from hulc2_amd.optim import lr_lambda_from_config  # noqa: E402
from hulc2_amd.trainer import ArenaTrainer, GradComm  # noqa: E402

BASE = 2e-4
LINEAR_2_OF_12 = {"_target_": "transformers.get_linear_schedule_with_warmup", "num_training_steps": 12, "num_warmup_steps": 2}


def _f32(x: float) -> float:
    return ctypes.c_float(x).value


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ulp32(x: float) -> float:
    a = torch.tensor(abs(x), dtype=torch.float32)
    return float((torch.nextafter(a, torch.tensor(float("inf"))) - a).double())


def _in_child(case: str) -> None:
    """run `_case_<case>(dev)` of this file in a fresh interpreter; its output is shown, a non-zero exit status fails the test"""
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), case], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, f"child `{case}` exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


def _model(dev, seed, dropout_p=0.1):
    kn.set_compute("bf16")
    m = instantiate(default_model_config(gripper_control=True, dropout_p=dropout_p)).to(dev)
    syn.fill_state_dict_(m.state_dict(), seed)
    m.train()
    return m


def _batch(dev, seed, B=2, S=8):
    b = syn.make_batch(seed, B, S, device=dev)
    for db in b.values():
        db.pop("plan_idx", None)
    return b


def _copy_into(dst, src) -> None:
    """overwrite the tensors of a (static) batch in place"""
    for k, v in src.items():
        if isinstance(v, dict):
            _copy_into(dst[k], v)
        else:
            dst[k].copy_(v)


# ---- 1. the kernel against torch on the CPU --------------------------------------------------------------------------------------------------
N = 100003                                                       # not a multiple of 4: the scalar tail of the pass runs too
SPECIALS = (0.0, -0.0, float("inf"), float("-inf"), float("nan"))


@functools.lru_cache(maxsize=None)
def _operands(n: int, count: int):
    """`count` seeded fp32 vectors of n elements: signs random, magnitudes log-uniform over 1e-30 .. 1e30 (normal numbers only; _expected
    asserts that no sum or scaled sum of them is subnormal either), with +-0, +-inf and NaN planted in every vector — at positions that
    meet each other across the vectors (inf + -inf, NaN + finite, -0 + 0, ...) and at positions of their own"""
    gen = torch.Generator().manual_seed(1000 * count + n % 997)
    out = []
    for t in range(count):
        mag = torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * 60.0 - 30.0).float()
        x = torch.where(torch.rand(n, generator=gen) < 0.5, -mag, mag)
        for i, s in enumerate(SPECIALS):
            if n:
                x[(i + t) % n] = s                                 # meets another vector's special at the head of the range (small n too)
            if n > 4096:
                x[n - 1 - (len(SPECIALS) * t + i)] = s             # its own place, inside the scalar tail's neighbourhood
                x[2048 + 17 * i + t] = SPECIALS[(i + 2 * t) % len(SPECIALS)]
        out.append(x)
    return tuple(out)


def _expected(gs, k):
    """the window on the CPU in fp32: k - 1 accumulations left to right, then (acc + g_k) * fp32(1 / k) — one add, one multiply"""
    acc = gs[0].clone()
    for g in gs[1:k - 1]:
        acc = acc + g
    out = (acc + gs[k - 1]) * torch.tensor(_f32(1.0 / k), dtype=torch.float32)
    for t in (acc, acc + gs[k - 1], out):                          # (whether a build keeps fp32 subnormals is not this file's question)
        assert not ((t != 0) & (t.abs() < 2.0 ** -126)).any(), "the operands must keep every intermediate value normal"
    return acc, out


def _assert_bits(got, want, what):
    got = got.cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaNs sit elsewhere"
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), \
        f"{what}: {int((_bits(got)[~nan] != _bits(want)[~nan]).sum())} of {got.numel()} elements differ in their bits"


def _window_on_device(dev, gs, k, n, offset=0):
    """store, add x (k - 2), finish on device copies (the launch covers [offset, offset + n)); checks what each mode must leave untouched"""
    acc = torch.full((offset + n,), 7.0, device=dev)               # (store must not read it: whatever is there is overwritten)
    acc_at_finish = None
    for j in range(k):
        g = gs[j].to(dev)
        before = g.clone()
        mode = "finish" if j == k - 1 else ("store" if j == 0 else "add")
        if mode == "finish":
            acc_at_finish = acc.clone()
        kn.grad_accumulate(acc[offset:], g[offset:], n, mode, _f32(1.0 / k) if mode == "finish" else 123.0)     # (scale is ignored outside finish)
        torch.cuda.synchronize()
        if mode == "finish":
            assert _same(acc, acc_at_finish), f"k={k}: finish must leave acc untouched"
            assert _same(g[:offset], before[:offset]), "elements in front of the range are not the launch's"
            return acc, g
        assert _same(g, before), f"k={k}: {mode} must leave g untouched"


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, N])
def test_kernel_matches_the_fp32_expression_on_the_cpu(dev, n):
    reached = set()
    for k in (2, 3, 7):
        gs = _operands(n, 7)[:k]
        want_acc, want_g = _expected(gs, k)
        acc, g = _window_on_device(dev, gs, k, n)
        _assert_bits(acc, want_acc, f"n={n} k={k}: the accumulator behind store / add")
        _assert_bits(g, want_g, f"n={n} k={k}: the finished gradient")
        reached |= {name for name, hit in (("nan", torch.isnan(want_g)), ("inf", torch.isinf(want_g)), ("zero", want_g == 0)) if hit.any()}
    if n == N:
        assert reached == {"nan", "inf", "zero"}, "the special values must reach the results"


def test_kernel_on_a_sub_range(dev):
    """one window launched on [4096, N) of both arenas: the head of the accumulator keeps its fill, the tail is the window's"""
    off = 4096
    for k in (2, 3):
        gs = _operands(N, 7)[:k]
        want_acc, want_g = _expected([g[off:] for g in gs], k)
        acc, g = _window_on_device(dev, gs, k, N - off, offset=off)
        assert float(acc[:off].min()) == 7.0 == float(acc[:off].max())
        _assert_bits(acc[off:], want_acc, f"sub-range k={k}: accumulator")
        _assert_bits(g[off:], want_g, f"sub-range k={k}: finished gradient")


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    a, g = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    bad = [lambda: kn.grad_accumulate(a, g, 64, 3),                                          # no such mode
           lambda: kn.grad_accumulate(a, g, 64, "mean"),
           lambda: kn.grad_accumulate(a, g, -1, "add"),
           lambda: kn.grad_accumulate(a, g, 65, "add"),                                      # longer than the tensors
           lambda: kn.grad_accumulate(a[1:], g, 32, "add"),                                  # a pointer offset by one element: not 16-byte aligned
           lambda: kn.grad_accumulate(a, g[1:], 32, "finish"),
           lambda: kn.grad_accumulate(a, a[16:], 32, "add"),                                 # overlapping ranges
           lambda: kn.grad_accumulate(a, a, 64, "store"),
           lambda: kn.grad_accumulate(a.double(), g.double(), 64, "add"),
           lambda: kn.grad_accumulate(a.bfloat16(), g.bfloat16(), 64, "add"),
           lambda: kn.grad_accumulate(a, g.double(), 64, "add"),
           lambda: kn.grad_accumulate(a.view(8, 8).t(), g, 64, "add"),                       # not contiguous
           lambda: kn.grad_accumulate(a.cpu(), g, 64, "add"),
           lambda: kn.grad_accumulate(a, g.cpu(), 64, "add")]
    accepted = []
    for i, call in enumerate(bad):
        try:
            call()
            accepted.append(i)
        except HulcKernelError:
            pass
    assert not accepted, f"calls {accepted} of the list were accepted"
    so = kn._L.load()                                                                        # the entry point's own codes, on device pointers
    assert so.hulc_grad_accumulate(a.data_ptr(), a.data_ptr() + 64, 32, 1, 1.0, None) == -2
    assert so.hulc_grad_accumulate(a.data_ptr() + 4, g.data_ptr(), 32, 1, 1.0, None) == -4
    assert so.hulc_grad_accumulate(a.data_ptr(), g.data_ptr(), 32, 3, 1.0, None) == -2
    torch.cuda.synchronize()
    assert float(a.abs().max()) == 0.0 and float(g.min()) == 1.0, "a refused call touches nothing"
    kn.grad_accumulate(a, g, 0, "store")                                                     # n == 0: a successful no-op
    kn.grad_accumulate(a, a[32:], 32, "store")                                               # neighbours that do not overlap are fine
    kn.grad_accumulate(a, g, 64, "add")
    torch.cuda.synchronize()
    assert float(a.min()) == 1.0 == float(a.max()), "store of zeros over zeros, then one add of ones"


# ---- 3. an eager window ------------------------------------------------------------------------------------------------------------------------
WINDOW_SEEDS = (21, 22, 23)


@functools.lru_cache(maxsize=None)
def _window_batches(dev):
    return tuple(_batch(dev, s) for s in WINDOW_SEEDS)


def _twin_gradients(dev):
    """a k = 1 trainer with lr = 0 on the window's seeds and batches: its parameters never move, so flat_g after its steps is g_1, g_2, g_3"""
    kn.reset_step_state(dev)
    m = _model(dev, 7)
    tr = ArenaTrainer(m, lr=0.0)
    try:
        p0, out = tr.flat_p.clone(), []
        for i, b in enumerate(_window_batches(dev)):
            tr.step(b, i)
            out.append(tr.flat_g.clone())
        torch.cuda.synchronize()
        assert _same(tr.flat_p, p0), "lr = 0: the twin's parameters never move"
        return out
    finally:
        tr.close()


def _adam_f64(p, g, m, v, lr32, t, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's update of one step in float64 from fp32 snapshots (weight decay 0, gradient scale 1) — the helper of
    tests/test_lr_schedule_gpu.py"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m1 = betas[0] * m + (1.0 - betas[0]) * g
    v1 = betas[1] * v + (1.0 - betas[1]) * g * g
    bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
    return p - (lr32 / bc1) * (m1 / (v1.sqrt() / (bc2 ** 0.5) + eps))


def _mean_of(gs):
    return ((gs[0] + gs[1]) + gs[2]) * torch.tensor(_f32(1.0 / 3), dtype=torch.float32, device=gs[0].device)


def test_eager_window_of_three(dev):
    """B=2, S=8, dropout 0.1, bf16 compute.  The twin runs twice (the control pair).  Where its two runs are bit-equal the accumulating
    trainer's arena behind the closing call equals ((g_1 + g_2) + g_3) * fp32(1/3), formed with torch fp32 ops from the twin's snapshots, bit
    for bit; otherwise it may differ from that by no more than the two control values differ.  Before the window closes nothing but the
    accumulator, the RNG word and the step count (bumped when the window opened) has changed; the closing call is ONE Adam step with t = 1
    on G, within 2^-24 |p| + 1e-5 lr of the float64 update (the bound of tests/test_lr_schedule_gpu.py).  A second window then moves the
    parameters again, by about lr."""
    twin_a, twin_b = _twin_gradients(dev), _twin_gradients(dev)
    want, want_b = _mean_of(twin_a), _mean_of(twin_b)
    control = float((want - want_b).abs().max())
    exact = all(_same(x, y) for x, y in zip(twin_a, twin_b))
    kn.reset_step_state(dev)
    rng0 = int(kn.step_state(dev)[0])
    tr = ArenaTrainer(_model(dev, 7), accumulate_grad_batches=3)
    try:
        batches = _window_batches(dev)
        p0, m0, v0 = tr.flat_p.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()
        words = []
        for j in (0, 1):
            assert tr.micro_batch == j
            loss = float(tr.step(batches[j], j))
            torch.cuda.synchronize()
            assert loss == loss
            assert _same(tr.flat_p, p0) and _same(tr.exp_avg, m0) and _same(tr.exp_avg_sq, v0) and tr._opt_steps == 0 and tr.step_count == 0
            words.append(kn.step_state(dev).tolist())
            assert words[-1][1] == 1, "the step count was bumped once, when the window opened"
        assert len({rng0, words[0][0], words[1][0]}) == 3, "every micro-batch walks the RNG word"
        assert _same(tr.flat_acc, twin_a[0] + twin_a[1]) or not exact
        assert tr.micro_batch == 2
        tr.step(batches[2], 2)
        torch.cuda.synchronize()
        assert tr.micro_batch == 0 and tr._opt_steps == 1 and tr.step_count == 1 and int(kn.step_state(dev)[1]) == 1
        G = tr.flat_g.clone()
        gap = float((G - want).abs().max())
        print(f"[eager window] control pair bit-equal: {exact} (max |difference| {control:.3e}); max |G - expected| = {gap:.3e}")
        if exact:
            assert _same(G, want), f"{int((_bits(G) != _bits(want)).sum())} elements of the finished arena differ from the twin's mean"
        else:
            assert gap <= control, (gap, control)
        assert not _same(G, twin_a[2]), "the optimizer must see the mean, not the last micro-batch's gradient"
        lr32 = _f32(BASE)
        upd = _adam_f64(p0, G, m0, v0, lr32, 1)
        excess = (tr.flat_p.double() - upd).abs() - (2.0 ** -24 * upd.abs() + 1e-5 * lr32)
        print(f"[eager window] max |p - float64 Adam(G)| - bound = {float(excess.max()):.3e}")
        assert float(excess.max()) <= 0.0, (float(excess.max()), int((excess > 0).sum()))
        # a second window
        p1 = tr.flat_p.clone()
        for j in range(3):
            tr.step(batches[j], j)
            torch.cuda.synchronize()
            assert _same(tr.flat_p, p1) == (j < 2)
        assert float((tr.flat_p - p1).abs().max()) > 0.5 * lr32 and tr._opt_steps == 2 and int(kn.step_state(dev)[1]) == 2
        assert not _same(tr.flat_g, twin_a[2])
    finally:
        tr.close()
        kn.reset_step_state(dev)


# ---- 4. k = 1 is today's trainer ------------------------------------------------------------------------------------------------------------
def test_a_window_of_one_is_the_plain_trainer(dev, monkeypatch):
    seen = []
    real = kn.grad_accumulate
    monkeypatch.setattr(kn, "grad_accumulate", lambda *a, **kw: (seen.append(a[3]), real(*a, **kw))[1])
    batch = _batch(dev, 9)

    def run(**kw):
        kn.reset_step_state(dev)
        tr = ArenaTrainer(_model(dev, 9), **kw)
        try:
            losses = [float(tr.step(batch, i)) for i in range(3)]
            torch.cuda.synchronize()
            assert tr.flat_acc is None and tr.micro_batch == 0 and tr._opt_steps == 3
            return losses, tr.flat_p.clone()
        finally:
            tr.close()

    (la, pa), (lb, pb) = run(accumulate_grad_batches=1), run()
    assert la == lb and _same(pa, pb)
    assert seen == [], "k = 1 never launches the accumulate pass"
    kn.reset_step_state(dev)


# ---- 5. the schedule and clipping count windows ---------------------------------------------------------------------------------------------
def test_schedule_and_clipping_go_by_windows(dev):
    f = lr_lambda_from_config(LINEAR_2_OF_12)
    kn.reset_step_state(dev)
    tr = ArenaTrainer(_model(dev, 9), accumulate_grad_batches=2, gradient_clip_val=0.5)
    try:
        tr.set_lr_schedule(f)
        batches = _window_batches(dev)
        for i in range(6):
            tr.step(batches[i % 3], i)
            assert tr._opt_steps == (i + 1) // 2 and tr.micro_batch == (i + 1) % 2
        torch.cuda.synchronize()
        assert tr._opt_steps == 3 and tr.step_count == 3
        assert float(tr._lr_dev) == _f32(BASE * f(2)), "the third optimizer step runs with the schedule's third factor"
        assert int(kn.step_state(dev)[1]) == 3
        want = float(tr.flat_g.double().pow(2).sum().sqrt())          # the finished arena of the closing call: G
        got = float(tr.grad_norm)
        print(f"[windows] grad_norm {got!r}, float64 norm of the finished arena {want!r}")
        assert want > 0 and abs(got - want) <= _ulp32(want)           # the bar of tests/test_grad_clip_gpu.py: 1 fp32 ulp of the float64 norm
    finally:
        tr.close()
        kn.reset_step_state(dev)


# ---- 6. graph mode ----------------------------------------------------------------------------------------------------------------------------
def test_graph_mode_replays_windows(dev):
    _in_child("graph_windows")


def _case_graph_windows(dev):
    """k = 2, B=4, S=16: two eager windows, capture(batch) (two warm-up windows), three windows of replay(), the static batch overwritten in
    place with new seeded data before every eager step and every replay.  Per window the parameters stay put behind the first replay and
    move by more than 0.5 lr behind the second, the step count grows by one, the graphs stay the same objects.  Against the same sequence
    run eagerly, under the control-pair rule of tests/test_lr_schedule_gpu.py::_case_eager_equals_replay: where a k = 1 pair (eager versus
    graph) is bit-equal in losses and flat_p the k = 2 pair must be too, otherwise its gap may be no larger than the control's."""
    B, S = 4, 16
    data = [_batch(dev, 30 + i, B, S) for i in range(3)]

    def run(k, graph, check=False):
        kn.reset_step_state(dev)
        tr = ArenaTrainer(_model(dev, 13), overlap=False, accumulate_grad_batches=k)
        batch = _batch(dev, 13, B, S)
        losses, fed = [], 0
        for i in range(2 * k):                                     # two eager windows
            _copy_into(batch, data[fed % 3])
            fed += 1
            losses.append(float(tr.step(batch, i)))
        if graph:
            tr.capture(batch)
            assert tr.micro_batch == 0, "capture() leaves the trainer at a window boundary"
        else:
            for i in range(2 * k):                                 # what capture() runs as its warm-up, on the batch as it stands
                tr.step(batch, i)
        torch.cuda.synchronize()
        assert tr._opt_steps == 4 and int(kn.step_state(dev)[1]) == 4
        g_fb, g_opt = tr.graph_fb, tr.graph_opt
        lr32 = _f32(BASE)
        for w in range(3):
            p_open = tr.flat_p.clone()
            for j in range(k):
                _copy_into(batch, data[fed % 3])
                fed += 1
                losses.append(float(tr.replay() if graph else tr.step(batch, 0)))
                torch.cuda.synchronize()
                if check:
                    assert tr.graph_fb is g_fb and tr.graph_opt is g_opt, "moving through a window must not drop or recapture a graph"
                    if j < k - 1:
                        assert _same(tr.flat_p, p_open) and tr.micro_batch == j + 1
                        with pytest.raises(RuntimeError, match="window boundary"):
                            tr.capture(batch)                      # (refused before it touches anything)
                    else:
                        moved = float((tr.flat_p - p_open).abs().max())
                        print(f"[graph windows] window {w}: max |dp| = {moved:.3e}, loss {losses[-1]:.6f}")
                        assert moved > 0.5 * lr32 and tr.micro_batch == 0
                    assert int(kn.step_state(dev)[1]) == 5 + w and tr._opt_steps == 4 + w + (j == k - 1)
        assert all(x == x for x in losses)
        kn.check_faults(dev)
        p = tr.flat_p.clone()
        tr.close()
        return losses, p

    def gap(x, y):
        return max(abs(a - b) for a, b in zip(x[0], y[0])), float((x[1] - y[1]).abs().max())

    c_e, c_g = run(1, False), run(1, True)
    a_e, a_g = run(2, False), run(2, True, check=True)
    control, acc = gap(c_e, c_g), gap(a_e, a_g)
    print(f"[graph windows] control gap (loss, p) = {control}, k = 2 gap = {acc}")
    if control == (0.0, 0.0) and torch.equal(c_e[1], c_g[1]):
        assert a_e[0] == a_g[0] and torch.equal(a_e[1], a_g[1]), (a_e[0], a_g[0], acc)
    else:
        assert acc[0] <= control[0] and acc[1] <= control[1], (acc, control)


# ---- 7. resume inside a window ------------------------------------------------------------------------------------------------------------------
def test_resume_inside_a_window(dev):
    """k = 3, stopped behind micro-batch 2: the state carries the running sum; a fresh model and trainer (a wrong lr, a scrambled step state)
    load it, run the remaining micro-batch and one whole window — losses and parameters are the uninterrupted run's, bit for bit"""
    batches = _window_batches(dev)
    kn.reset_step_state(dev)
    m = _model(dev, 9)
    tr = ArenaTrainer(m, accumulate_grad_batches=3)
    for j in range(2):
        tr.step(batches[j], j)
    model_sd = {k: v.clone() for k, v in m.state_dict().items()}
    opt_sd = tr.state_dict()
    assert opt_sd["accumulate"]["k"] == 3 and opt_sd["accumulate"]["position"] == 2
    assert set(opt_sd["accumulate"]["sum"]) == {n for n, p in m.named_parameters() if p.requires_grad}
    want = [float(tr.step(batches[j % 3], j)) for j in range(2, 6)]
    torch.cuda.synchronize()
    p_want = tr.flat_p.clone()
    assert tr._opt_steps == 2 and tr.micro_batch == 0
    tr.close()
    kn.reset_step_state(dev, seed=12345)                           # whatever the process did in between
    m2 = _model(dev, 1)
    tr2 = ArenaTrainer(m2, lr=1.0, accumulate_grad_batches=3)      # (a wrong rate: the checkpoint's must win)
    try:
        m2.load_state_dict(model_sd)
        tr2.load_state_dict(opt_sd)
        assert tr2.micro_batch == 2 and tr2._opt_steps == 0
        got = [float(tr2.step(batches[j % 3], j)) for j in range(2, 6)]
        torch.cuda.synchronize()
        assert tr2._opt_steps == 2 and tr2.micro_batch == 0 and int(kn.step_state(dev)[1]) == 2
        assert got == want, (got, want)
        assert _same(tr2.flat_p, p_want)
    finally:
        tr2.close()
        kn.reset_step_state(dev)


# ---- 8. one exchange per window (RCCL, one rank) ------------------------------------------------------------------------------------------------
def test_one_exchange_per_window_on_the_rccl_path(dev):
    _in_child("rccl_single_rank")


def _case_rccl_single_rank(dev):
    """process group "nccl" with one rank and force_comm=True, as tests/test_ddp_gpu.py::test_rccl_path_executes_single_rank sets the RCCL
    path up: overlap=False, k = 2, eager windows and then captured ones (the split graphs of several ranks).  A spy on GradComm.reduce sees
    nothing behind the opening micro-batch and the arena exactly once behind the closing one."""
    import socket
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        calls = []
        real = GradComm.reduce

        def spy(self, lo, hi, async_op=False):
            calls.append((lo, hi))
            return real(self, lo, hi, async_op)
        GradComm.reduce = spy
        kn.reset_step_state(dev)
        with pytest.raises(ValueError, match="overlap=False"):
            ArenaTrainer(torch.nn.Linear(8, 8).to(dev), force_comm=True, overlap=True, accumulate_grad_batches=2)   # (refused before it builds anything)
        tr = ArenaTrainer(_model(dev, 13), force_comm=True, overlap=False, accumulate_grad_batches=2)
        assert tr.multi and tr.comm.active and calls == [], "one rank: no probe of the fabric at construction"
        batch = _batch(dev, 13, 4, 16)

        def covered():
            spans, calls[:] = sorted(calls), []
            return spans

        for w in range(2):                                         # eager
            tr.step(batch, 0)
            assert covered() == [], "no exchange behind the opening micro-batch"
            tr.step(batch, 1)
            assert covered() == [(0, tr.total)], "one exchange of the whole arena per window"
        tr.capture(batch)
        assert covered() == [(0, tr.total)] * 2, "the two warm-up windows of capture()"
        assert tr.graph_enc is not None, "several ranks: the split graphs"
        p = tr.flat_p.clone()
        for w in range(2):                                         # captured
            tr.replay()
            torch.cuda.synchronize()
            assert covered() == [] and _same(tr.flat_p, p)
            tr.replay()
            torch.cuda.synchronize()
            assert covered() == [(0, tr.total)] and not _same(tr.flat_p, p)
            p = tr.flat_p.clone()
        kn.check_faults(dev)
        assert tr._opt_steps == 6 and int(kn.step_state(dev)[1]) == 6
        tr.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    globals()["_case_" + sys.argv[1]](torch.device("cuda", 0))
