"""The KL weight as a device scalar that captured graphs follow (reference: hulc2/utils/kl_callbacks.py -> Hulc2.set_kl_beta every epoch), on
the GPU:
  * the four *_sched entry points give the bits of their scalar twins when the device word holds the same fp32 value, and follow the word
    when only IT is rewritten between launches; beta = 0 gives exact zeros
  * a missing / misaligned beta_dev is refused (-1 / -4) and nothing is written
  * CatKLFn forward + backward captured as one graph follows the word from replay to replay
  * the step node captures once and replays through an annealing sequence, bit-equal to the eager node
  * ArenaTrainer.replay() follows ArenaTrainer.set_kl_beta, bit-equal to a trainer stepping eagerly; a by-value capture refuses a changed weight

Dropout is off, plan indices / noise are injected, seeds are fixed.  The cases that capture graphs run in a child process each, as in
tests/test_lr_schedule_gpu.py (the suite's later step-node tests see the same number of earlier captures with or without this file)."""
import ctypes
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
pytestmark = pytest.mark.gpu

from hulc2_amd import functional as HF, kernels as kn, lib, switches, synthetic as syn  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402
from hulc2_amd.lib import HulcKernelError  # noqa: E402

BETAS = (0.0, 2.4726230185478927e-05, 0.01, 1.0)                 # sigmoid(10, 50, 0.01) at epoch 10 is the second one
ANNEAL = (0.0, 2.47e-05, 0.005, 0.01)
MIX = 0.8
WRONG = 123.0                                                    # the by-value beta of every *_sched call: must be ignored


def _f32(x: float) -> float:
    return ctypes.c_float(x).value


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got: dict, want: dict, what):
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), f"{what}: {k} differs (max |diff| {float((got[k] - want[k]).abs().max()):.3e})"


def _in_child(case: str) -> None:
    """run `_case_<case>(dev)` of this file in a fresh interpreter; its output is shown, a non-zero exit status fails the test"""
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), case], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, f"child `{case}` exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


# ---- 1. kernels: discrete KL ------------------------------------------------------------------------------------------------------------------
def _cat_inputs(dev, B, G, nseg):
    g = torch.Generator().manual_seed(1000 * B + 10 * G + nseg)
    pp, pr = torch.randn(B, G * 32, generator=g).to(dev), torch.randn(B, G * 32, generator=g).to(dev)
    gout = (0.5 + torch.rand(nseg, generator=g)).to(dev)
    return pp, pr, gout


def _cat_run(pp, pr, gout, B, G, nseg, beta, beta_dev=None):
    """forward + backward launches -> {out, kl_group, dpp, dpr}; outputs start as NaN: every element must be written"""
    nan = lambda *s: torch.full(s, float("nan"), device=pp.device)  # noqa: E731
    out, klg, dpp, dpr = nan(nseg), nan(B * G), nan(B, G * 32), nan(B, G * 32)
    kn.cat_kl_fwd(pp, pr, B, G, 32, beta, out, klg, nseg, beta_dev=beta_dev)
    kn.cat_kl_bwd(pp, pr, klg, B, G, 32, beta, MIX, gout, dpp, dpr, nseg, beta_dev=beta_dev)
    torch.cuda.synchronize()
    return {"out": out, "kl_group": klg, "dpp": dpp, "dpr": dpr}


# (2, 3, *): 6 groups in an 8-group block — a tail block; (4, 32, 2): the configured 32 categories, 16 blocks
@pytest.mark.parametrize("B,G,nseg", [(2, 3, 1), (2, 3, 2), (4, 32, 2)])
def test_cat_kl_sched_gives_the_scalar_bits_and_follows_the_word(dev, B, G, nseg):
    pp, pr, gout = _cat_inputs(dev, B, G, nseg)
    word = torch.zeros(1, device=dev)
    scalar = {}
    for beta in BETAS:
        scalar[beta] = _cat_run(pp, pr, gout, B, G, nseg, beta)
        assert all(torch.isfinite(v).all() for v in scalar[beta].values())
        word.fill_(_f32(beta))
        _same_bits(_cat_run(pp, pr, gout, B, G, nseg, WRONG, beta_dev=word), scalar[beta], f"beta {beta}")
    z = scalar[0.0]
    assert (z["out"] == 0).all() and (z["dpp"] == 0).all() and (z["dpr"] == 0).all() and (z["kl_group"] > 0).all()
    assert not torch.equal(scalar[0.01]["out"], scalar[1.0]["out"]) and not torch.equal(scalar[0.01]["dpr"], scalar[1.0]["dpr"])
    # only the device word changes between these launches: the host arguments stay what they were
    args = (pp, pr, gout, B, G, nseg, WRONG)
    for beta in (1.0, 0.01, 2.4726230185478927e-05, 0.0):
        word.fill_(_f32(beta))
        _same_bits(_cat_run(*args, beta_dev=word), scalar[beta], f"word rewritten to {beta}")


# ---- 2. kernels: continuous plan --------------------------------------------------------------------------------------------------------------
def _gauss_inputs(dev, B, P, nseg):
    g = torch.Generator().manual_seed(2000 * B + 10 * P + nseg)
    pp, pr = torch.randn(B, 2 * P, generator=g).to(dev), torch.randn(B, 2 * P, generator=g).to(dev)
    eps, dplan = torch.randn(B, P, generator=g).to(dev), torch.randn(B, P, generator=g).to(dev)
    gout = (0.5 + torch.rand(nseg, generator=g)).to(dev)
    return pp, pr, eps, dplan, gout


def _gauss_run(pp, pr, eps, dplan, gout, B, P, nseg, beta, beta_dev=None):
    nan = lambda *s: torch.full(s, float("nan"), device=pp.device)  # noqa: E731
    plan, out, klr, dpp, dpr = nan(B, P), nan(nseg), nan(B), nan(B, 2 * P), nan(B, 2 * P)
    kn.gauss_plan_fwd(pp, pr, eps, 7, B, P, beta, nseg, plan, None, out, klr, beta_dev=beta_dev)
    kn.gauss_plan_bwd(pp, pr, eps, 7, B, P, beta, MIX, nseg, dplan, gout, dpp, dpr, beta_dev=beta_dev)
    torch.cuda.synchronize()
    return {"plan": plan, "out": out, "kl_row": klr, "dpp": dpp, "dpr": dpr}


@pytest.mark.parametrize("with_dplan", [True, False], ids=["dplan", "no-dplan"])
@pytest.mark.parametrize("B,P,nseg", [(2, 3, 1), (2, 3, 2), (4, 256, 2)])       # P = 3: an odd feature count, the last lane's pair is half empty
def test_gauss_plan_sched_gives_the_scalar_bits_and_follows_the_word(dev, B, P, nseg, with_dplan):
    pp, pr, eps, dplan, gout = _gauss_inputs(dev, B, P, nseg)
    dplan = dplan if with_dplan else None
    word = torch.zeros(1, device=dev)
    scalar = {}
    for beta in BETAS:
        scalar[beta] = _gauss_run(pp, pr, eps, dplan, gout, B, P, nseg, beta)
        assert all(torch.isfinite(v).all() for v in scalar[beta].values())
        word.fill_(_f32(beta))
        _same_bits(_gauss_run(pp, pr, eps, dplan, gout, B, P, nseg, WRONG, beta_dev=word), scalar[beta], f"beta {beta}")
    z = scalar[0.0]
    assert (z["out"] == 0).all() and (z["dpp"] == 0).all() and (z["kl_row"] > 0).all()
    if not with_dplan:
        assert (z["dpr"] == 0).all()
    assert not torch.equal(scalar[0.01]["out"], scalar[1.0]["out"]) and not torch.equal(scalar[0.01]["dpp"], scalar[1.0]["dpp"])
    args = (pp, pr, eps, dplan, gout, B, P, nseg, WRONG)
    for beta in (1.0, 0.01, 2.4726230185478927e-05, 0.0):
        word.fill_(_f32(beta))
        _same_bits(_gauss_run(*args, beta_dev=word), scalar[beta], f"word rewritten to {beta}")


def test_gauss_sample_only_calls_take_no_beta_dev(dev):
    """out == None / gout == None: beta is not read, the *_sched entries run without a pointer and give the sample-only bits"""
    B, P = 2, 3
    pp, pr, eps, dplan, _ = _gauss_inputs(dev, B, P, 1)
    so = lib.load()
    res = []
    for fwd, bwd in ((so.hulc_gauss_plan_fwd, so.hulc_gauss_plan_bwd), (so.hulc_gauss_plan_fwd_sched, so.hulc_gauss_plan_bwd_sched)):
        tail = (None,) if fwd is so.hulc_gauss_plan_fwd_sched else ()
        plan, dpr = torch.full((B, P), float("nan"), device=dev), torch.full((B, 2 * P), float("nan"), device=dev)
        torch.cuda.synchronize()
        assert fwd(None, pr.data_ptr(), eps.data_ptr(), 7, None, B, P, 1e-4, 0.0, 1, plan.data_ptr(), None, None, None, *tail, None) == 0
        assert bwd(None, pr.data_ptr(), eps.data_ptr(), 7, None, B, P, 1e-4, 0.0, 0.0, 1, dplan.data_ptr(), None, None, dpr.data_ptr(),
                   *tail, None) == 0
        torch.cuda.synchronize()
        res.append({"plan": plan, "dpr": dpr})
    assert torch.isfinite(res[0]["plan"]).all() and torch.isfinite(res[0]["dpr"]).all()
    _same_bits(res[1], res[0], "sample-only")


# ---- 3. guards --------------------------------------------------------------------------------------------------------------------------------
def test_null_and_misaligned_beta_dev_are_refused_and_nothing_is_written(dev):
    B, G, P = 2, 3, 3
    so = lib.load()
    so.hulc_last_error.restype = ctypes.c_char_p
    pp, pr, gout = _cat_inputs(dev, B, G, 1)
    qp, qr, eps, dplan, _ = _gauss_inputs(dev, B, P, 1)
    word = torch.zeros(4, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    outs = [nan(1), nan(B * G), nan(B, G * 32), nan(B, G * 32), nan(B, P), nan(B), nan(B, 2 * P), nan(B, 2 * P)]
    out, klg, dpp, dpr, plan, klr, dqp, dqr = outs
    klg_in = torch.zeros(B * G, device=dev)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()  # noqa: E731
    for bad, rc, msg in ((None, -1, "null beta_dev"), (p(word) + 2, -4, "beta_dev must be 4-byte aligned")):
        calls = {
            "hulc_cat_kl_fwd_sched": (p(pp), p(pr), B, G, 32, 0.5, 1, p(out), p(klg), bad, None),
            "hulc_cat_kl_bwd_sched": (p(pp), p(pr), p(klg_in), B, G, 32, 0.5, MIX, p(gout), 1, p(dpp), p(dpr), bad, None),
            "hulc_gauss_plan_fwd_sched": (p(qp), p(qr), p(eps), 7, None, B, P, 1e-4, 0.5, 1, p(plan), None, p(out), p(klr), bad, None),
            "hulc_gauss_plan_bwd_sched": (p(qp), p(qr), p(eps), 7, None, B, P, 1e-4, 0.5, MIX, 1, p(dplan), p(gout), p(dqp), p(dqr), bad, None),
        }
        for name, args in calls.items():
            assert getattr(so, name)(*args) == rc, name
            assert so.hulc_last_error().decode() == f"{name}: {msg}"
    # the operand checks the two entries of a pair share name the entry that was called
    assert so.hulc_cat_kl_fwd_sched(None, p(pr), B, G, 32, 0.5, 1, p(out), p(klg), p(word), None) == -1
    assert so.hulc_last_error().decode() == "hulc_cat_kl_fwd_sched: null pointer"
    assert so.hulc_cat_kl_fwd(None, p(pr), B, G, 32, 0.5, 1, p(out), p(klg), None) == -1
    assert so.hulc_last_error().decode() == "hulc_cat_kl_fwd: null pointer"
    assert so.hulc_cat_kl_bwd_sched(p(pp), p(pr), p(klg_in), B, G, 16, 0.5, MIX, p(gout), 1, p(dpp), p(dpr), p(word), None) == -2
    assert so.hulc_last_error().decode() == "hulc_cat_kl_bwd_sched: class_size must be 32"
    assert so.hulc_gauss_plan_fwd_sched(p(qp), p(qr), p(eps), 7, None, B, P, 1e-4, 0.5, 1, None, None, None, None, p(word), None) == -1
    assert so.hulc_last_error().decode() == "hulc_gauss_plan_fwd_sched: nothing to compute (plan, eps_out and out are all null)"
    assert so.hulc_gauss_plan_bwd_sched(p(qp), p(qr), p(eps), 7, None, B, P, 1e-4, 0.5, MIX, 1, None, None, p(dqp), p(dqr), p(word), None) == -1
    assert so.hulc_last_error().decode() == "hulc_gauss_plan_bwd_sched: nothing to compute (dplan and gout are both null)"
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in outs), "a refused call writes nothing"
    # the Python wrappers take a one-element fp32 tensor on the operands' device and nothing else
    for wrong in (0.5, torch.zeros(2, device=dev), torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1)):
        with pytest.raises(HulcKernelError, match="beta_dev"):
            kn.cat_kl_fwd(pp, pr, B, G, 32, 0.5, out, klg, 1, beta_dev=wrong)
        with pytest.raises(HulcKernelError, match="beta_dev"):
            kn.cat_kl_bwd(pp, pr, klg_in, B, G, 32, 0.5, MIX, gout, dpp, dpr, 1, beta_dev=wrong)
        with pytest.raises(HulcKernelError, match="beta_dev"):
            kn.gauss_plan_fwd(qp, qr, eps, 7, B, P, 0.5, 1, plan, None, out, klr, beta_dev=wrong)
        with pytest.raises(HulcKernelError, match="beta_dev"):
            kn.gauss_plan_bwd(qp, qr, eps, 7, B, P, 0.5, MIX, 1, dplan, gout, dqp, dqr, beta_dev=wrong)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in outs)


# ---- 4. the model's device word -------------------------------------------------------------------------------------------------------------
def _model(dev, seed):
    kn.set_compute("bf16")
    m = instantiate(default_model_config(gripper_control=True, dropout_p=0.0)).to(dev)
    syn.fill_state_dict_(m.state_dict(), seed)
    m.train()
    return m


def test_set_kl_beta_on_a_gpu_model(dev, monkeypatch):
    """by value until the first call; then a plain-attribute device word (no state_dict key) that compute_kl_loss reads: the scalar path's
    bits, and the oracle's value within fp32 rounding of the sums (1e-5 relative: 1024 terms of ~2^-24 each, and libm's exp / log)"""
    from hulc2_amd.utils.distributions import DiscState
    from oracle import hulc2_oracle as O

    m = _model(dev, 3)
    keys = set(m.state_dict())
    g = torch.Generator().manual_seed(9)
    pp, pr = torch.randn(4, 1024, generator=g), torch.randn(4, 1024, generator=g)
    sp, sr = DiscState(pp.to(dev)), DiscState(pr.to(dev))
    assert not m.kl_beta_on_device and m._kl_beta_arg() == 0.01
    before = m.compute_kl_loss(sp, sr)
    m.set_kl_beta(0.00025)
    assert m.kl_beta == 0.00025 and type(m.kl_beta) is float and m.kl_beta_on_device
    w = m._kl_beta_dev
    assert w.shape == (1,) and w.dtype == torch.float32 and w.device == sp.logit.device and float(w) == _f32(0.00025)
    assert m._kl_beta_arg() is w
    assert set(m.state_dict()) == keys and not any(b is w for b in m.buffers()) and not any(q is w for q in m.parameters())
    got = m.compute_kl_loss(sp, sr)
    want = m.dist.kl_balanced(sp, sr, 0.00025, m.kl_balancing_mix)              # by value
    assert torch.equal(_bits(got.reshape(1)), _bits(want.reshape(1))) and not torch.equal(got, before)
    ref = O.kl_loss(pp.double(), pr.double(), 0.00025, m.kl_balancing_mix)
    assert abs(float(got) - float(ref)) <= 1e-5 * float(ref), (float(got), float(ref))
    m.set_kl_beta(0.01)
    assert m._kl_beta_dev is w, "later calls write the same word"
    assert torch.equal(_bits(m.compute_kl_loss(sp, sr).reshape(1)), _bits(before.reshape(1)))
    # a value set while the model is on the CPU must not leave the old word behind when the model comes back
    m.cpu()
    assert not m.kl_beta_on_device and m._kl_beta_arg() == 0.01
    m.set_kl_beta(0.002)
    assert m._kl_beta_arg() == 0.002
    m.to(dev)
    assert m.kl_beta_on_device
    w2 = m._kl_beta_arg()
    assert w2 is w and float(w2) == _f32(0.002) and m.kl_beta == 0.002
    m.set_kl_beta(0.01)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)     # (as inside torch.cuda.graph, without capturing here)
    with pytest.raises(RuntimeError, match="stream capture"):
        m.set_kl_beta(0.5)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert m.kl_beta == 0.01 and float(w) == _f32(0.01)


# ---- 5. one captured forward + backward -------------------------------------------------------------------------------------------------------
def test_a_captured_kl_node_follows_the_device_word(dev):
    _in_child("captured_node")


def _case_captured_node(dev):
    """CatKLFn forward and backward captured as ONE graph (a single chain: no parallel branches); three values written into the word, each
    replay bit-equal to eager scalar launches"""
    B, G, nseg = 4, 32, 2
    pp, pr, gout = _cat_inputs(dev, B, G, nseg)
    pp.requires_grad_(True)
    pr.requires_grad_(True)
    word = torch.full((1,), _f32(0.5), device=dev)

    def fwd_bwd():
        out = HF.CatKLFn.apply(pp, pr, G, 32, word, MIX, nseg)
        return (out,) + torch.autograd.grad(out, (pp, pr), grad_outputs=gout)

    torch.cuda.synchronize()
    side = kn.capture_stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd_bwd()                                                  # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with kn.no_gc():
        with torch.cuda.graph(graph, stream=side):
            out, dpp, dpr = fwd_bwd()
    torch.cuda.synchronize()
    seen = []
    for beta in (0.01, 0.0, 2.4726230185478927e-05):
        word.fill_(_f32(beta))
        graph.replay()
        torch.cuda.synchronize()
        want = _cat_run(pp.detach(), pr.detach(), gout, B, G, nseg, beta)
        _same_bits({"out": out, "dpp": dpp, "dpr": dpr}, {k: want[k] for k in ("out", "dpp", "dpr")}, f"replay with beta {beta}")
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[2]) and (seen[1] == 0).all()

    # Hulc2.set_kl_beta inside a real stream capture raises before anything is written (a Hulc2 with one GPU parameter: the method reads
    # nothing else of the model)
    from hulc2_amd.models.hulc2 import Hulc2
    m = Hulc2.__new__(Hulc2)
    torch.nn.Module.__init__(m)
    m.anchor = torch.nn.Parameter(torch.zeros(1, device=dev))
    m.kl_beta = 0.01
    m.set_kl_beta(0.25)
    torch.cuda.synchronize()
    other = torch.cuda.CUDAGraph()
    with kn.no_gc():
        with torch.cuda.graph(other, stream=side):
            kept = word * 2.0                                      # (the capture holds one node of its own)
            with pytest.raises(RuntimeError, match="stream capture"):
                m.set_kl_beta(0.5)
    torch.cuda.synchronize()
    assert m.kl_beta == 0.25 and float(m._kl_beta_dev) == 0.25
    other.replay()
    torch.cuda.synchronize()
    assert float(m._kl_beta_dev) == 0.25 and float(kept) == 2.0 * float(word), "the refused call left nothing in the graph"


# ---- 6. the step node ---------------------------------------------------------------------------------------------------------------------------
def test_step_node_replays_through_an_annealing_sequence(dev):
    _in_child("step_node")


def _anneal_loop(dev):
    """the reference's loop shape: set_kl_beta at the start of each of four 'epochs' of two steps (SGD, no autocast)
    -> (node, losses, [{name: .grad} per step], captures after each epoch)"""
    kn.reset_step_state(dev)
    m = _model(dev, 43)
    batch = syn.make_batch(43, 2, 8, device=dev)                  # (plan_idx stays in: the plan sample is injected)
    params = [p for p in m.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-3)
    named = list(m.named_parameters())
    losses, grads, captures = [], [], []
    for epoch, beta in enumerate(ANNEAL):
        m.set_kl_beta(beta)
        for i in range(2):
            opt.zero_grad(set_to_none=True)
            loss = m.training_step(batch, 2 * epoch + i)
            loss.backward()
            grads.append({n: (None if p.grad is None else p.grad.detach().clone()) for n, p in named})
            opt.step()
            losses.append(float(loss))
        captures.append(m.__dict__["_hulc_step_node"].captures)
    torch.cuda.synchronize()
    kn.check_faults(dev)
    return m.__dict__["_hulc_step_node"], losses, grads, captures


def _case_step_node(dev):
    """Two steps per epoch, beta = 0, 2.47e-5, 0.005, 0.01 set before each epoch.  The node takes its two eager steps in the first epoch,
    captures ONCE at the third call and replays the other six calls: the captures never increase after that one (with beta in the signature
    every epoch was a new layout: nothing was ever captured, or — with longer epochs — every epoch captured again).  Loss and every parameter
    gradient of every step are bit-equal to the same loop on the eager node (HULC_NO_STEP_GRAPH=1)."""
    with switches.scope(HULC_NO_STEP_NODE=None, HULC_NO_STEP_GRAPH="1"):
        ne, le, ge, ce = _anneal_loop(dev)
    assert ce == [0, 0, 0, 0] and ne.eager_steps == 8
    with switches.scope(HULC_NO_STEP_NODE=None, HULC_NO_STEP_GRAPH=None):
        ng, lg, gg, cg = _anneal_loop(dev)
    assert ng.disabled is None, ng.disabled
    print(f"[step node] captures after each epoch {cg}; eager {ng.eager_steps}, replays {ng.replays}, evictions {ng.evictions}")
    assert cg == [0, 1, 1, 1], cg
    assert (ng.captures, ng.eager_steps, ng.replays, ng.evictions) == (1, 2, 6, 0)
    assert len(set(le)) == 8 or le[0] != le[7], "the run must move"
    assert lg == le, (lg, le)
    for i, (a, b) in enumerate(zip(gg, ge)):
        assert a.keys() == b.keys()
        bad = [n for n in a if (a[n] is None) != (b[n] is None) or (a[n] is not None and not torch.equal(_bits(a[n]), _bits(b[n])))]
        assert not bad, f".grad after the backward of step {i}: {len(bad)} of {len(a)} tensors differ, e.g. {bad[:3]}"


# ---- 7. the native loop -----------------------------------------------------------------------------------------------------------------------
def test_arena_trainer_replay_follows_set_kl_beta(dev):
    _in_child("native_loop")


def _case_native_loop(dev):
    """capture() after set_kl_beta(0.0), then four replays with beta = 0, 2.47e-5, 0.005, 0.01 set through ArenaTrainer.set_kl_beta: all
    parameters after every step bit-equal to a twin trainer taking the same steps eagerly.  (Before the weight was a device scalar replay()
    kept the beta of the capture: the parameters differed from the second replay on.)  Then a capture with beta by value: replay() refuses a
    changed model.kl_beta by name, and ArenaTrainer.set_kl_beta drops those graphs once."""
    from hulc2_amd.trainer import ArenaTrainer

    def run(graph):
        kn.reset_step_state(dev)
        m = _model(dev, 17)
        tr = ArenaTrainer(m, overlap=False)
        batch = syn.make_batch(17, 2, 8, device=dev)
        tr.set_kl_beta(0.0)
        assert m.kl_beta_on_device
        if graph:
            tr.capture(batch)
            fb, opt = tr.graph_fb, tr.graph_opt
        else:
            for i in range(2):                                     # capture()'s two warm-up steps
                tr.step(batch, i)
        ps, losses = [], []
        for beta in ANNEAL:
            tr.set_kl_beta(beta)
            losses.append(float(tr.replay() if graph else tr.step(batch, 0)))
            torch.cuda.synchronize()
            ps.append(tr.flat_p.clone())
            if graph:
                assert tr.graph_fb is fb and tr.graph_opt is opt, "a change of the KL weight must not drop or recapture a graph"
        kn.check_faults(dev)
        return losses, ps

    le, pe = run(False)
    lg, pg = run(True)
    print(f"[native loop] eager losses {le}\n[native loop] replay losses {lg}")
    for k, (a, b) in enumerate(zip(pg, pe)):
        n = int((_bits(a) != _bits(b)).sum())
        assert n == 0, f"after step {k} (beta {ANNEAL[k]}): {n} of {a.numel()} parameters differ, max |diff| {float((a - b).abs().max()):.3e}"
    assert lg == le, (lg, le)
    assert not torch.equal(pe[0], pe[3])

    # a capture with beta by value cannot see a later model.kl_beta: loud
    kn.reset_step_state(dev)
    m = _model(dev, 17)
    tr = ArenaTrainer(m, overlap=False)
    batch = syn.make_batch(17, 2, 8, device=dev)
    tr.capture(batch)
    assert not m.kl_beta_on_device and tr._kl_captured == 0.01
    tr.replay()
    m.set_kl_beta(0.005)
    with pytest.raises(RuntimeError, match=r"ArenaTrainer\.set_kl_beta.*capture\(\)"):
        tr.replay()
    tr.set_kl_beta(0.005)                                          # the switch to the device word drops the by-value graphs, once
    assert tr.graph_fb is None and tr.graph_opt is None and tr._kl_captured is None
    with pytest.raises(RuntimeError, match="no captured graphs"):
        tr.replay()
    torch.cuda.synchronize()
    kn.check_faults(dev)


if __name__ == "__main__":
    assert torch.cuda.is_available()
    globals()["_case_" + sys.argv[1]](torch.device("cuda:0"))
