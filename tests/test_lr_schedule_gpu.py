"""A learning-rate schedule in every training loop (reference: hulc2/models/hulc2.py:160-198, `interval: step`), on the GPU:
  * hulc_adam_step_sched reads the learning rate from device memory and gives the bits of the scalar-argument entry points
  * a captured launch follows the device scalar from replay to replay
  * ArenaTrainer.set_lr_schedule: eager steps and graph replays run with base_lr * lr_lambda(k), checked against a float64 recomputation
  * state_dict / load_state_dict continue the sequence; the reference loop (configure_optimizers + hulc2_amd.optim.Adam) follows its scheduler

The cases that capture graphs run in a child process each (`_in_child`): graph launches of this HIP runtime have died depending on how many
captures the process had made before (NOTES "Round 6", what the fork / join took besides), and the step-node tests that follow in the
suite's process should see the same number of earlier captures with or without this file."""
import ctypes
import subprocess
import sys
import types
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
pytestmark = pytest.mark.gpu

from hulc2_amd import kernels as kn, synthetic as syn  # noqa: E402
from hulc2_amd.compat import Config, instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402
from hulc2_amd.lib import HulcKernelError  # noqa: E402
from hulc2_amd.optim import lr_lambda_from_config  # noqa: E402
from hulc2_amd.trainer import ArenaTrainer  # noqa: E402

BASE = 2e-4
LINEAR_2_OF_12 = {"_target_": "transformers.get_linear_schedule_with_warmup", "num_training_steps": 12, "num_warmup_steps": 2}
COSINE = {"_target_": "transformers.get_cosine_schedule_with_warmup", "num_training_steps": -1, "num_warmup_steps": 0.1, "num_cycles": 0.5}


def _f32(x: float) -> float:
    return ctypes.c_float(x).value


def _in_child(case: str) -> None:
    """run `_case_<case>(dev)` of this file in a fresh interpreter; its output is shown, a non-zero exit status fails the test"""
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), case], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, f"child `{case}` exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


def _model(dev, seed, dropout_p=0.1, lr_scheduler=None):
    kn.set_compute("bf16")
    cfg = default_model_config(gripper_control=True, dropout_p=dropout_p)
    if lr_scheduler is not None:
        cfg["lr_scheduler"] = Config.wrap(dict(lr_scheduler))
    m = instantiate(cfg).to(dev)
    syn.fill_state_dict_(m.state_dict(), seed)
    m.train()
    return m


def _batch(dev, seed, B=2, S=8):
    b = syn.make_batch(seed, B, S, device=dev)
    for db in b.values():
        db.pop("plan_idx", None)
    return b


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------
N = 100003                                                       # not a multiple of 4: the scalar tail of the pass runs too
LO_RANGES = ((0, 4096), (50000, N))
FACTORS = (0.0, 0.25, 0.5, 1.0, 0.7)


class _Arena:
    def __init__(self, p0, dev):
        self.p = p0.clone().to(dev)
        self.m, self.v = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        self.shadow = torch.zeros(N, dtype=torch.bfloat16, device=dev)
        self.lo = torch.zeros(N, dtype=torch.bfloat16, device=dev)

    def tensors(self):
        return {"p": self.p, "m": self.m, "v": self.v, "shadow": self.shadow, "lo": self.lo}

    def step(self, g, lr, step, **kw):
        kn.adam_step(self.p, g, self.m, self.v, self.shadow, N, lr, 0.9, 0.999, 1e-8, 0.0, step, lo=self.lo, lo_ranges=LO_RANGES, **kw)


def _same_bits(a: _Arena, b: _Arena, what):
    for (k, x), y in zip(a.tensors().items(), b.tensors().values()):
        assert torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int16),
                           y.view(torch.int32 if y.dtype == torch.float32 else torch.int16)), f"{what}: {k} differs"


@pytest.mark.parametrize("mode", ["host_step", "device_step", "amp"])
def test_device_lr_gives_the_bits_of_the_scalar_argument(dev, mode):
    """Five steps with learning rates 2e-4 * {0, 0.25, 0.5, 1, 0.7}: one arena driven through lr_dev (its scalar argument a wrong number, to
    show it is ignored), its twin through the scalar argument of today's entry points — p, m, v, the bf16 shadow and the remainders are the
    same bits after every step.  `amp`: with the GradScaler's device scalars, the third step skipped (found_inf set).  The same steps against
    torch.optim.Adam in float64 with those learning rates: the bound of test_adam_kernel_matches_torch (1.5e-6, fp32 rounding of O(1)
    parameters) holds unchanged, no factor exceeds 1 so no update is larger than there."""
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(N, generator=gen)
    grads = [torch.randn(N, generator=gen) * (10.0 ** (i - 2)) for i in range(5)]
    ref = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.Adam([ref], lr=BASE)
    a, b = _Arena(p0, dev), _Arena(p0, dev)
    lr_dev = torch.zeros(1, device=dev)
    words = torch.zeros(2, dtype=torch.int64, device=dev)          # {unused, step count} as hulc2_amd.optim.Adam keeps them
    S = 65536.0
    scale, found = torch.full((1,), S, device=dev), torch.zeros(1, device=dev)
    taken = 0
    for i, (gr, fac) in enumerate(zip(grads, FACTORS)):
        lr = BASE * fac
        skip = mode == "amp" and i == 2
        kw = {}
        if mode == "amp":
            found.fill_(1.0 if skip else 0.0)
            kw.update(loss_scale_dev=scale, found_inf_dev=found)
            gr_dev = (gr * S).to(dev)                               # (a power of two: exact)
        else:
            gr_dev = gr.to(dev)
        if mode != "host_step":
            kn.step_count_advance_if(words, found if mode == "amp" else None)
            kw.update(step_state_dev=words)
        if not skip:
            taken += 1
            opt.param_groups[0]["lr"] = lr
            ref.grad = gr.double()
            opt.step()
        before = {k: t.clone() for k, t in a.tensors().items()}
        lr_dev.fill_(_f32(lr))
        a.step(gr_dev, 123.0, max(taken, 1), lr_dev=lr_dev, **kw)
        b.step(gr_dev, lr, max(taken, 1), **kw)
        torch.cuda.synchronize()
        _same_bits(a, b, f"{mode} step {i}")
        if skip:
            assert all(torch.equal(t, before[k]) for k, t in a.tensors().items()), "a skipped step leaves everything untouched"
        elif fac == 0.0:
            assert torch.equal(a.p, before["p"]) and not torch.equal(a.m, before["m"]), "lr 0 moves the moments, not the parameters"
    if mode != "host_step":
        assert int(words[1]) == taken
    err = (a.p.double().cpu() - ref.detach()).abs().max().item()
    print(f"[lr_dev kernel, {mode}] max |p - float64 torch.optim.Adam| after 5 steps: {err:.3e}")
    assert err < 1.5e-6, f"Adam parameters after 5 scheduled steps: max err {err:.3e}"
    assert torch.equal(a.shadow, a.p.to(torch.bfloat16))
    inside = torch.zeros(N, dtype=torch.bool, device=dev)
    for lo, hi in LO_RANGES:
        inside[lo:hi] = True
    want_lo = (a.p - a.shadow.float()).to(torch.bfloat16)
    assert torch.equal(a.lo[inside], want_lo[inside]) and float(a.lo[~inside].float().abs().max()) == 0.0


def test_lr_dev_of_the_wrong_kind_is_refused(dev):
    a = _Arena(torch.zeros(N), dev)
    g = torch.zeros(N, device=dev)
    for bad in (torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float16, device=dev),
                torch.zeros(2, device=dev), torch.zeros(1)):
        with pytest.raises(HulcKernelError):
            a.step(g, BASE, 1, lr_dev=bad)
    a.step(g, BASE, 1, lr_dev=torch.full((1,), BASE, device=dev))  # (and the right kind is taken)
    torch.cuda.synchronize()


# ---- 2. one captured launch ---------------------------------------------------------------------------------------------------------------
def test_a_captured_launch_follows_the_device_scalar(dev):
    _in_child("captured_launch")


def _case_captured_launch(dev):
    """One adam_step(lr_dev=t, step_state_dev=words) captured as a graph and replayed six times, a new learning rate written into t and the
    step word advanced before each replay: the bits of six eager launches that take the learning rate as the scalar argument."""
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(N, generator=gen)
    grads = [torch.randn(N, generator=gen) for _ in range(6)]
    lrs = [BASE * f for f in (0.0, 0.5, 1.0, 0.9, 0.35, 0.1)]
    a, b = _Arena(p0, dev), _Arena(p0, dev)
    g_static = torch.zeros(N, device=dev)
    t = torch.zeros(1, device=dev)
    wa, wb = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    kn.fault_word(dev)                                             # (lazily made device word: must exist before the capture)
    torch.cuda.synchronize()
    side = kn.capture_stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with kn.no_gc():
        with torch.cuda.graph(graph, stream=side):
            a.step(g_static, 123.0, 1, lr_dev=t, step_state_dev=wa)
    torch.cuda.synchronize()
    assert torch.equal(a.p.cpu(), p0), "a capture runs nothing"
    for gr, lr in zip(grads, lrs):
        gd = gr.to(dev)
        g_static.copy_(gd)
        t.fill_(_f32(lr))
        kn.step_count_advance_if(wa, None)
        graph.replay()
        kn.step_count_advance_if(wb, None)
        b.step(gd, lr, 1, step_state_dev=wb)
        torch.cuda.synchronize()
        _same_bits(a, b, f"replay with lr {lr}")
    assert int(wa[1]) == 6 and not torch.equal(a.p.cpu(), p0)


# ---- 3. / 4. / 5. the native loop ------------------------------------------------------------------------------------------------------------
def _adam_f64(p, g, m, v, lr32, t, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's update of one step in float64 from fp32 snapshots (weight decay 0, gradient scale 1)"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m1 = betas[0] * m + (1.0 - betas[0]) * g
    v1 = betas[1] * v + (1.0 - betas[1]) * g * g
    bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
    return p - (lr32 / bc1) * (m1 / (v1.sqrt() / (bc2 ** 0.5) + eps))


def test_graph_replay_follows_the_schedule(dev):
    _in_child("graph_replay")


def _case_graph_replay(dev):
    """Graph mode, checked without the code under test: B=4, S=16, linear warm-up over 2 of 12 steps.  Two eager steps (k = 0, 1), capture()
    (its own two warm-up steps are k = 2, 3), six replays (k = 4 .. 9, factors 0.8 .. 0.3).  For every replay the update is recomputed in
    float64 from snapshots of the arenas, with fp32(base_lr * lr_lambda(k)) and the DEVICE step word for the bias corrections, and
    |flat_p - expected| <= 2^-24 |p| + 1e-5 lr_k per element: half an ulp for the final rounding plus about ten fp32 roundings inside an
    update no larger than about 10 lr.  A run that ignored the schedule would miss this by ~0.5 lr ~ 1e-4 on most elements."""
    f = lr_lambda_from_config(LINEAR_2_OF_12)
    kn.reset_step_state(dev)
    m = _model(dev, 13, 0.1)
    tr = ArenaTrainer(m, overlap=False)
    tr.set_lr_schedule(f)
    batch = _batch(dev, 13, B=4, S=16)
    p0, m0 = tr.flat_p.clone(), tr.exp_avg.clone()
    tr.step(batch, 0)                                              # k = 0: factor 0
    torch.cuda.synchronize()
    assert f(0) == 0.0 and torch.equal(tr.flat_p, p0), "the first step of a warm-up runs with lr 0: parameters bit-unchanged"
    assert not torch.equal(tr.exp_avg, m0), "... while the moments move"
    tr.step(batch, 1)
    assert float(tr._lr_dev) == _f32(BASE * f(1)) and not torch.equal(tr.flat_p, p0)
    tr.capture(batch)
    assert tr._opt_steps == 4 and int(kn.step_state(dev)[1]) == 4
    g_opt, g_fb = tr.graph_opt, tr.graph_fb
    worst = 0.0
    for k in range(4, 10):
        torch.cuda.synchronize()
        p, m1, v1 = tr.flat_p.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()
        loss = float(tr.replay())
        torch.cuda.synchronize()
        assert loss == loss
        lr32 = _f32(BASE * f(k))
        assert float(tr._lr_dev) == lr32 and tr.lr == BASE * f(k), (k, float(tr._lr_dev), lr32)
        t = int(kn.step_state(dev)[1])
        assert t == k + 1
        want = _adam_f64(p, tr.flat_g, m1, v1, lr32, t)
        excess = (tr.flat_p.double() - want).abs() - (2.0 ** -24 * want.abs() + 1e-5 * lr32)
        moved = float((tr.flat_p - p).abs().max())
        print(f"[graph schedule] k={k} lr={lr32:.3e} max |p - expected| - bound = {float(excess.max()):.3e}, max |dp| = {moved:.3e}")
        worst = max(worst, float(excess.max()))
        assert moved > 0.5 * lr32, "the step must have moved the parameters by about lr"
        assert float(excess.max()) <= 0.0, (k, float(excess.max()), int((excess > 0).sum()))
        assert tr.graph_opt is g_opt and tr.graph_fb is g_fb, "a change of learning rate must not drop or recapture a graph"
    assert tr._opt_steps == 10


def test_scheduled_eager_steps_equal_scheduled_replays(dev):
    _in_child("eager_equals_replay")


def _case_eager_equals_replay(dev):
    """The same schedule through step() only and through step() x 2, capture() (two more steps), replay() x 4, next to a control pair without
    a schedule on the same seeds.  Where the control pair is bit-equal (losses and flat_p) the scheduled pair must be too; where it is not,
    that is how eager and replayed steps of this configuration already relate, and the scheduled pair may differ by no more than the control
    pair does (max |difference| of the losses and of flat_p)."""
    f = lr_lambda_from_config(LINEAR_2_OF_12)

    def run(scheduled, graph):
        kn.reset_step_state(dev)
        m = _model(dev, 13, 0.1)
        tr = ArenaTrainer(m, overlap=False)
        if scheduled:
            tr.set_lr_schedule(f)
        batch = _batch(dev, 13, B=4, S=16)
        losses = [float(tr.step(batch, i)) for i in range(2)]
        if graph:
            tr.capture(batch)
            losses += [float(tr.replay()) for _ in range(4)]
        else:
            for i in range(2):
                tr.step(batch, i)
            losses += [float(tr.step(batch, 0)) for _ in range(4)]
        torch.cuda.synchronize()
        assert tr._opt_steps == 8
        return losses, tr.flat_p.clone()

    def gap(x, y):
        return max(abs(a - b) for a, b in zip(x[0], y[0])), float((x[1] - y[1]).abs().max())

    c_e, c_g = run(False, False), run(False, True)
    s_e, s_g = run(True, False), run(True, True)
    assert s_e[0] != c_e[0], "the schedule must change the run"
    control, sched = gap(c_e, c_g), gap(s_e, s_g)
    print(f"[eager vs replay] control gap (loss, p) = {control}, scheduled gap = {sched}")
    if control == (0.0, 0.0) and torch.equal(c_e[1], c_g[1]):
        assert s_e[0] == s_g[0] and torch.equal(s_e[1], s_g[1]), (s_e[0], s_g[0], sched)
    else:
        assert sched[0] <= control[0] and sched[1] <= control[1], (sched, control)


def test_resume_continues_the_schedule(dev):
    f = lr_lambda_from_config(LINEAR_2_OF_12)
    batch = _batch(dev, 9)
    kn.reset_step_state(dev)
    m = _model(dev, 9, 0.1)
    tr = ArenaTrainer(m)
    tr.set_lr_schedule(f)
    for i in range(3):
        tr.step(batch, i)
    model_sd = {k: v.clone() for k, v in m.state_dict().items()}
    opt_sd = tr.state_dict()
    assert opt_sd["lr_schedule"] == {"base_lr": BASE, "position": 3, "device_lr": True}
    group = tr.to_torch_adam_state_dict()["param_groups"][0]
    assert group["initial_lr"] == BASE and group["lr"] == BASE * f(3) and 0.0 < group["lr"] < BASE
    want = [float(tr.step(batch, i)) for i in range(3, 6)]
    p_want = tr.flat_p.clone()
    kn.reset_step_state(dev, seed=12345)                           # whatever the process did in between
    m2 = _model(dev, 1, 0.1)
    tr2 = ArenaTrainer(m2, lr=1.0)                                 # (a wrong base rate: the checkpoint's must win)
    m2.load_state_dict(model_sd)
    tr2.load_state_dict(opt_sd)
    tr2.set_lr_schedule(f)
    got = [float(tr2.step(batch, i)) for i in range(3, 6)]
    torch.cuda.synchronize()
    assert tr2._opt_steps == 6 and float(tr2._lr_dev) == _f32(BASE * f(5))
    assert got == want, (got, want)
    assert torch.equal(tr2.flat_p, p_want)


# ---- 6. the reference's loop ------------------------------------------------------------------------------------------------------------------
def test_reference_loop_follows_the_configured_scheduler(dev):
    _in_child("reference_loop")


def _case_reference_loop(dev):
    """configure_optimizers() with the cosine config (40 steps from the trainer stub -> 4 warm-up steps) and the drop-in hulc2_amd.optim.Adam:
    six iterations of training_step -> backward -> optimizer.step() -> scheduler.step() -> zero_grad() (the step node captures its graphs at
    the third call).  The arena kernel is launched six times with the transformers sequence of learning rates; the first one (factor 0)
    leaves the parameters as they were; the end is bit-equal to a model driven with the same rates set by hand and no scheduler."""
    import os
    import transformers
    from hulc2_amd.optim import Adam
    for k in ("HULC_TORCH_ADAM", "HULC_NO_STEP_NODE", "HULC_NO_STEP_GRAPH"):     # (this process is the case's own)
        os.environ.pop(k, None)
    probe = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=BASE)
    g = transformers.get_cosine_schedule_with_warmup(probe, num_warmup_steps=4, num_training_steps=40, num_cycles=0.5).lr_lambdas[0]
    want_lrs = [BASE * g(k) for k in range(6)]
    assert want_lrs[0] == 0.0 and want_lrs[4] == BASE and want_lrs[5] < BASE
    seen = []
    real = kn.adam_step

    def spy(*args, **kw):
        seen.append(args[6])
        return real(*args, **kw)
    kn.adam_step = spy                                            # (hulc2_amd.optim calls it through the module)

    def loop(with_scheduler):
        kn.reset_step_state(dev)
        m = _model(dev, 19, 0.1, lr_scheduler=COSINE if with_scheduler else None)
        m.trainer = types.SimpleNamespace(estimated_stepping_batches=40)
        batch = _batch(dev, 19)
        out = m.configure_optimizers()
        opt, sched = out["optimizer"], out["lr_scheduler"]["scheduler"]
        assert isinstance(opt, Adam)
        p0 = [p.detach().clone() for p in m.parameters()]
        del seen[:]
        for i in range(6):
            if not with_scheduler:
                opt.param_groups[0]["lr"] = want_lrs[i]
            loss = m.training_step(batch, i)
            loss.backward()
            opt.step()
            if with_scheduler:
                sched.step()
            if i == 0:
                torch.cuda.synchronize()
                assert all(torch.equal(a, b.detach()) for a, b in zip(p0, m.parameters())), "factor 0: parameters bit-unchanged"
            opt.zero_grad()
        torch.cuda.synchronize()
        kn.check_faults(dev)
        assert opt.fused_launches == 6
        assert seen == want_lrs, (seen, want_lrs)
        assert m.__dict__["_hulc_step_node"].replays >= 3
        return [p.detach().clone() for p in m.parameters()], p0

    p_sched, p0 = loop(True)
    p_hand, _ = loop(False)
    assert any(not torch.equal(a, b) for a, b in zip(p_sched, p0))
    assert all(torch.equal(a, b) for a, b in zip(p_sched, p_hand))


if __name__ == "__main__":
    globals()["_case_" + sys.argv[1]](torch.device("cuda", 0))
