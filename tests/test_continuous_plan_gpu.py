"""The continuous (diagonal Gaussian) latent plan, conf/model/distribution/continuous.yaml, at the model level: Hulc2 trains, validates and
rolls out with Distribution(dist="continuous"), on the eager Functions, the step node, its replayed graphs and ArenaTrainer.

The oracle does not know this mode: the float64 restatements below are built on torch.distributions from the reference formulas
(hulc2/utils/distributions.py:28-29,55-59, hulc2/models/hulc2.py:235-237,444-466).  Tolerance rule: tests/kcheck.py, margin LIBM = 4.

The cases that capture graphs run in a child process each (`_in_child`, as in tests/test_lr_schedule_gpu.py): graph launches of this HIP
runtime have died depending on how many captures the process had made before, and the step-node tests that follow in the suite's process
should see the same number of earlier captures with or without this file."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.distributions import Independent, Normal, kl_divergence

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
pytestmark = pytest.mark.gpu

from hulc2_amd import kernels as kn, switches, synthetic as syn  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402
from tests.kcheck import EPS32, compare  # noqa: E402

MARGIN = 4.0                       # the LIBM row of tests/test_losses_gpu.py
MIN_STD = 1e-4
P = 256


@pytest.fixture(autouse=True)
def _bf16_afterwards():
    yield
    kn.set_compute("bf16")


def _in_child(case: str) -> None:
    """run `_case_<case>(dev)` of this file in a fresh interpreter; its output is shown, a non-zero exit status fails the test"""
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), case], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, f"child `{case}` exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


def _model(dev, seed, dropout_p=0.0, distribution="continuous", gripper_control=True):
    m = instantiate(default_model_config(gripper_control=gripper_control, dropout_p=dropout_p, distribution=distribution)).to(dev)
    syn.fill_state_dict_(m.state_dict(), seed)
    m.train()
    return m


def _batch(dev, seed, B=2, S=8, eps=True):
    b = syn.make_batch(seed, B, S, device=dev)
    for name, db in b.items():
        db.pop("plan_idx", None)
        if eps:
            db["plan_eps"] = torch.randn(B, P, generator=syn._gen(seed, "plan_eps." + name)).to(dev)
    return b


def _state(raw):
    mean, r = torch.chunk(raw, 2, dim=-1)
    return mean, F.softplus(r) + MIN_STD


def _dist(mean, std):
    return Independent(Normal(mean, std), 1)


def _balanced_kl(pp, pr, beta, mix, nseg):
    """hulc2.py:444-466 on raw head outputs, one value per segment"""
    (mp, sp), (mq, sq) = _state(pp), _state(pr)
    lhs = kl_divergence(_dist(mq.detach(), sq.detach()), _dist(mp, sp))
    rhs = kl_divergence(_dist(mq, sq), _dist(mp.detach(), sp.detach()))
    return beta * (mix * lhs.view(nseg, -1).mean(1) + (1.0 - mix) * rhs.view(nseg, -1).mean(1))


def _standin(dt):
    """Distribution.rsample_plan_and_kl in plain torch at precision dt: raw tensors cast to dt, sample and balanced KL, cast back"""
    def node(self, pp_state, pr_state, seed, idx, kl_beta, mix, nseg=1, eps=None):
        pp, pr = pp_state.raw.to(dt), pr_state.raw.to(dt)
        mean, std = _state(pr)
        plan = mean + std * eps.to(dt)                       # Normal.rsample with the injected noise
        return plan.float(), None, _balanced_kl(pp, pr, kl_beta, mix, nseg).float()
    return node


def _step(m, batch):
    for p in m.parameters():
        p.grad = None
    loss = m.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
    logged = {k: torch.as_tensor(v).detach().double().cpu().clone() for k, v in m.logged.items() if k.startswith("train/")}
    return loss.detach().clone(), grads, logged


def test_built_step_equals_the_float64_stand_in(dev, monkeypatch):
    """fp32 compute mode, eager Function path, plan_eps injected, dropout 0: the step as built against the same step with the fused node
    replaced by a float64 torch.distributions node; the yardstick e_ref is the same stand-in in float32.  Every parameter gradient (relative
    L2) and every logged loss within 4 * max(e_ref, 2^-23)."""
    from hulc2_amd.utils.distributions import Distribution

    kn.set_compute("fp32")
    m = _model(dev, 5)
    batch = _batch(dev, 5)
    _, g_built, l_built = _step(m, batch)
    assert "_hulc_step_node" not in m.__dict__, "fp32 mode runs the eager Functions"
    monkeypatch.setattr(Distribution, "rsample_plan_and_kl", _standin(torch.float64))
    _, g64, l64 = _step(m, batch)
    monkeypatch.setattr(Distribution, "rsample_plan_and_kl", _standin(torch.float32))
    _, g32, l32 = _step(m, batch)
    monkeypatch.undo()
    assert set(l_built) == set(l64) and any("kl_loss" in k for k in l64)
    bad = []
    for k in sorted(l64):
        ref = l64[k].abs().max().item()
        err, e_ref = (l_built[k] - l64[k]).abs().max().item() / ref, (l32[k] - l64[k]).abs().max().item() / ref
        print(f"[standin] {k:40s} built {err:.3e}  f32 stand-in {e_ref:.3e}")
        if err > MARGIN * max(e_ref, EPS32):
            bad.append((k, err, e_ref))
    for n in sorted(g64):
        assert (g_built[n] is None) == (g64[n] is None) == (g32[n] is None), n
        if g64[n] is None:
            continue
        ref = g64[n].double().norm().item()
        assert ref > 0, n
        err = (g_built[n].double() - g64[n].double()).norm().item() / ref
        e_ref = (g32[n].double() - g64[n].double()).norm().item() / ref
        print(f"[standin] g {n:70s} built {err:.3e}  f32 stand-in {e_ref:.3e}")
        if err > MARGIN * max(e_ref, EPS32):
            bad.append((n, err, e_ref))
    assert not bad, f"{len(bad)} tensors beyond {MARGIN:g} * max(e_ref, 2^-23): {bad[:6]}"


def _same(a, b, what):
    assert a.keys() == b.keys()
    bad = []
    for n in a:
        if a[n] is None or b[n] is None:
            if not (a[n] is None and b[n] is None):
                bad.append((n, "None on one side"))
        elif not torch.equal(a[n], b[n]):
            bad.append((n, float((a[n] - b[n]).abs().max())))
    assert not bad, f"{what}: {len(bad)} tensors differ, e.g. {bad[:4]}"


def test_eager_node_step_node_and_replayed_graphs_give_the_same_bits(dev):
    _in_child("same_bits")


def _case_same_bits(dev):
    """bf16 mode, the same batch with plan_eps injected and unchanged weights through the eager node (HULC_NO_STEP_GRAPH=1), the step node
    before its capture (calls 0 and 1) and its replayed graphs (calls 2 and 3): losses and all gradients bit for bit"""
    kn.set_compute("bf16")

    def run(calls, **env):
        with switches.scope(HULC_NO_STEP_NODE=None, **env):
            kn.reset_step_state(dev)
            m = _model(dev, 31)
            batch = _batch(dev, 31)
            out = [_step(m, batch) for _ in range(calls)]
        return m.__dict__["_hulc_step_node"], out

    node_e, eager = run(1, HULC_NO_STEP_GRAPH="1")
    assert node_e.captures == 0 and node_e.eager_steps == 1
    node, graphed = run(4, HULC_NO_STEP_GRAPH=None)
    assert node.disabled is None, node.disabled
    assert node.captures == 1 and node.replays == 2 and node.eager_steps == 2, (node.captures, node.replays, node.eager_steps)
    l0, g0, logs0 = eager[0]
    for i, (l, g, logs) in enumerate(graphed):
        what = "the step node before capture" if i < 2 else "the replayed graphs"
        assert torch.equal(l, l0), (what, i, float(l), float(l0))
        assert logs.keys() == logs0.keys() and all(torch.equal(logs[k], logs0[k]) for k in logs0), (what, i)
        _same(g, g0, f"{what}, call {i}, against the eager node")


def test_arena_trainer_captures_and_replays_the_continuous_step(dev):
    _in_child("arena_trainer")


def _case_arena_trainer(dev):
    """no plan_eps: the noise comes from the counter RNG at the device step word.  Losses finite, two trainers from the same seed agree bit for
    bit (steps, capture, replays), successive replays draw different plans"""
    from hulc2_amd.trainer import ArenaTrainer

    kn.set_compute("bf16")

    def run():
        kn.reset_step_state(dev)
        m = _model(dev, 13, dropout_p=0.1)
        tr = ArenaTrainer(m, overlap=False)
        batch = _batch(dev, 13, B=4, S=16, eps=False)
        plan_now = torch.zeros(8, P, device=dev)
        inner = m.action_decoder.loss_stacked

        def tap(plan, *a, **kw):
            plan_now.copy_(plan.detach())                    # (inside the capture: a copy node of the graph)
            return inner(plan, *a, **kw)
        m.action_decoder.loss_stacked = tap
        losses = [float(tr.step(batch, i)) for i in range(2)]
        tr.capture(batch)
        plans = []
        for _ in range(4):
            losses.append(float(tr.replay()))
            torch.cuda.synchronize()
            plans.append(plan_now.clone())
        kn.check_faults(dev)
        weights = tr.flat_p.clone()
        tr.close()
        return losses, plans, weights

    l1, p1, w1 = run()
    l2, p2, w2 = run()
    assert all(np.isfinite(l1)), l1
    assert l1 == l2, (l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(p1, p2)) and torch.equal(w1, w2)
    assert all(torch.isfinite(p).all() and p.abs().max() > 0 for p in p1)
    for a, b in zip(p1[:-1], p1[1:]):
        assert not torch.equal(a, b), "successive replays must draw different plans (the noise follows the device step word)"


def test_aten_ops_of_a_continuous_training_step(dev):
    """tests/test_launch_count_gpu.py for the continuous configuration: same allowed set, at most 6 framework ops"""
    from aten_trace import launches
    from hulc2_amd.trainer import ArenaTrainer

    kn.set_compute("bf16")
    model = _model(dev, 42, dropout_p=0.1)
    tr = ArenaTrainer(model, lr=2e-4, overlap=False)
    batch = _batch(dev, 42, B=32, S=32, eps=False)
    for i in range(3):
        tr.step(batch, i)
    rows = launches(lambda: tr.step(batch, 3))
    listing = "\n".join(f"{op:16s} {shp} {where}" for op, shp, where in rows)
    print(listing)
    big = [r for r in rows if any(len(s) and torch.Size(s).numel() >= 1 << 20 for s in r[1])]
    assert not big, "a framework op touches a large tensor on the hot path:\n" + "\n".join(map(str, big))
    allowed = {"add", "add_", "cat", "clone"}
    other = [r for r in rows if r[0] not in allowed]
    assert not other, "unexpected framework ops on the hot path:\n" + "\n".join(map(str, other))
    assert len(rows) <= 6, f"{len(rows)} framework ops per step:\n" + listing
    tr.close()


def test_validation_step_and_rollout(dev):
    """validation_step with plan_eps_pp / plan_eps_pr: the returned plans are mean + std * eps of the prior's / posterior's states, val_kl
    is the float64 KL of those states; reset / step run with both goal kinds"""
    kn.set_compute("bf16")
    m = _model(dev, 11, dropout_p=0.1)
    m.eval()
    B, S = 2, 8
    batch = _batch(dev, 3, B, S, eps=False)
    for name, db in batch.items():
        db["plan_eps_pp"] = torch.randn(B, P, generator=syn._gen(3, "eps_pp." + name)).to(dev)
        db["plan_eps_pr"] = torch.randn(B, P, generator=syn._gen(3, "eps_pr." + name)).to(dev)
    states = {"pp": [], "pr": []}
    hooks = [m.plan_proposal.register_forward_hook(lambda mod, i, o: states["pp"].append(o)),
             m.plan_recognition.register_forward_hook(lambda mod, i, o: states["pr"].append(o[0]))]
    out = m.validation_step(batch, 0)
    for h in hooks:
        h.remove()
    from hulc2_amd.utils.distributions import ContState
    for i, mod in enumerate(("vis", "lang")):
        db = batch[mod]
        for kind in ("pp", "pr"):
            st = states[kind][i]
            assert isinstance(st, ContState)
            raw = st.raw.detach().cpu()
            eps = db[f"plan_eps_{kind}"].cpu()
            ref = [(lambda ms: ms[0] + ms[1] * eps.to(dt))(_state(raw.to(dt))) for dt in (torch.float64, torch.float32)]
            got = out[f"sampled_plan_{kind}_{mod}"]
            assert got.shape == (B, P)
            compare("validation_step", f"plan_{kind}_{mod}", got, ref[0], ref[1], MARGIN)
            mean, std = st
            assert torch.equal(mean, st.raw[:, :P]) and torch.equal(std, F.softplus(st.raw[:, P:]) + MIN_STD)
        pp, pr = states["pp"][i].raw.detach().cpu(), states["pr"][i].raw.detach().cpu()
        kl = [_balanced_kl(pp.to(dt), pr.to(dt), m.kl_beta, m.kl_balancing_mix, 1) for dt in (torch.float64, torch.float32)]
        compare("validation_step", f"val_kl_{mod}", torch.as_tensor(m.logged[f"val_kl/{mod}_kl_loss"]).reshape(1), kl[0], kl[1], MARGIN)
        assert out[f"idx_{mod}"].shape[0] == B
    for k in ("val_act/vis_act_loss_pp", "val_act/lang_act_loss_pr", "val_total_mae/lang_total_mae_pp", "val_grip/vis_grip_sr_pr",
              "val/val_pred_clip_loss", "val_act/action_loss_pp"):
        assert torch.isfinite(torch.as_tensor(m.logged[k])).all(), k
    m.replan_freq = 2
    m.reset()
    vis = batch["vis"]
    goal = {"lang": batch["lang"]["lang"][:1]}
    plans = []
    for s in range(4):
        obs = {"rgb_obs": {k: v[:1, s:s + 1] for k, v in vis["rgb_obs"].items()}, "depth_obs": {},
               "robot_obs": vis["robot_obs"][:1, s:s + 1], "robot_obs_raw": vis["state_info"]["robot_obs"][:1, s:s + 1]}
        a = m.step(obs, goal)
        assert a.shape == (1, 1, 7) and torch.isfinite(a).all()
        assert m.plan.shape == (1, P) and torch.isfinite(m.plan).all()
        plans.append(m.plan.clone())
    assert torch.equal(plans[0], plans[1]) and torch.equal(plans[2], plans[3]), "the plan is kept between replans"
    assert not torch.equal(plans[1], plans[2]), "a replan draws a new plan"
    m.reset()
    gobs = {"rgb_obs": {k: v[:1, -1:] for k, v in vis["rgb_obs"].items()}, "depth_obs": {}, "robot_obs": vis["robot_obs"][:1, -1:]}
    obs = {"rgb_obs": {k: v[:1, :1] for k, v in vis["rgb_obs"].items()}, "depth_obs": {}, "robot_obs": vis["robot_obs"][:1, :1],
           "robot_obs_raw": vis["state_info"]["robot_obs"][:1, :1]}
    a = m.step(obs, gobs)
    assert a.shape == (1, 1, 7) and torch.isfinite(a).all() and m.plan.shape == (1, P)


def test_the_discrete_config_still_gives_the_golden_losses(dev):
    """guards the dispatch: the discrete model, built in this process after the continuous ones, against tests/golden/step_B2_S16.npz at the
    bf16 loss tolerance of tests/test_parity_gpu.py"""
    fx = dict(np.load(ROOT / "tests" / "golden" / "step_B2_S16.npz", allow_pickle=False))
    vs = dict(np.load(ROOT / "tests" / "golden" / "vision_static.npz", allow_pickle=False))
    kn.set_compute("bf16")
    m = _model(dev, int(vs["seed"]), distribution="discrete", gripper_control=False)
    batch = syn.make_batch(int(fx["seed"]), 2, 16, device=dev)
    total = m.training_step(batch, 0)
    tol = 2e-4
    for got, key in ((total, "total_loss"), (m.logged["train/kl_loss"], "kl_loss"), (m.logged["train/action_loss"], "action_loss"),
                     (m.logged["train/lang_clip_loss"] / 3.0, "clip_loss")):
        got, ref = float(got), float(fx[key])
        assert abs(got - ref) <= tol * abs(ref) + 1e-6, (key, got, ref)


if __name__ == "__main__":
    globals()["_case_" + sys.argv[1]](torch.device("cuda", 0))
