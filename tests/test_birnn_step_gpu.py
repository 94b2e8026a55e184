"""One training step of Hulc2 with the recurrent posterior (default_model_config(posterior="birnn")), B = 2 per modality, S = 8, with the
discrete and the continuous plan, in all three loops:

  * the eager step in fp32 compute against the CPU oracle's pieces (oracle/hulc2_oracle.py: encoders, goal encoders, prior, sample, KL,
    decoder, contrastive loss) with tests/birnnref.module_forward as the posterior, in float64: the total loss and the posterior's 18
    gradients under the fp32 bars of tests/test_parity_gpu.py (discrete plan: the oracle has no Gaussian plan);
  * the step node: its eager form, the calls before its capture and its replayed graphs give the same loss, logged values and every
    gradient bit for bit, as tests/test_stepnode_gpu.py asserts for the default model;
  * ArenaTrainer: a trainer that only steps and one that steps, captures and replays agree bit for bit on losses, the gradient arena and
    the parameters;
  * validation_step runs (eval mode) and returns finite values.
kn.check_faults follows each.  The cases that capture graphs run in a child process each, as in tests/test_continuous_plan_gpu.py."""
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
pytestmark = pytest.mark.gpu

from hulc2_amd import kernels as kn, switches, synthetic as syn  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402

B, S = 2, 8
DISTS = ["discrete", "continuous"]


@pytest.fixture(autouse=True)
def _bf16_afterwards():
    yield
    kn.set_compute("bf16")


def _in_child(case: str, dist: str) -> None:
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), case, dist], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, f"child `{case} {dist}` exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


def _model(dev, seed, dist):
    m = instantiate(default_model_config(gripper_control=True, dropout_p=0.0, distribution=dist, posterior="birnn")).to(dev)
    syn.fill_state_dict_(m.state_dict(), seed)
    m.train()
    return m


def _batch(dev, seed, dist, inject=True):
    b = syn.make_batch(seed, B, S, device=dev)
    for name, db in b.items():
        if dist == "continuous" or not inject:
            db.pop("plan_idx", None)
        if dist == "continuous" and inject:
            db["plan_eps"] = torch.randn(B, 256, generator=syn._gen(seed, "plan_eps." + name)).to(dev)
    return b


def _step(m, batch):
    for p in m.parameters():
        p.grad = None
    loss = m.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    kn.check_faults(loss.device)
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
    logged = {k: torch.as_tensor(v).detach().double().cpu().clone() for k, v in m.logged.items() if k.startswith("train/")}
    return loss.detach().clone(), grads, logged


def _same(a, b, what):
    assert a.keys() == b.keys()
    bad = [(n, "None on one side" if (a[n] is None or b[n] is None) else float((a[n] - b[n]).abs().max())) for n in a
           if (a[n] is None) != (b[n] is None) or (a[n] is not None and not torch.equal(a[n], b[n]))]
    assert not bad, f"{what}: {len(bad)} tensors differ, e.g. {bad[:4]}"


def _oracle_step(sd, batch):
    """oracle.hulc2_oracle.training_step with the recurrent posterior in place of the transformer's: -> total loss (float64 autograd graph)"""
    from oracle import hulc2_oracle as O
    from tests import birnnref as R

    cfg = dict(gripper_control=True)
    total = clip = 0.0
    post = {k[len("plan_recognition."):]: v for k, v in sd.items() if k.startswith("plan_recognition.")}
    for m, db in batch.items():
        emb = O.concat_encoders(sd, "perceptual_encoder.", db["rgb_static"], db["rgb_gripper"])
        goal = O.language_goal_encoder(sd, "language_goal.", db["lang"]) if "lang" in m else O.visual_goal_encoder(sd, "visual_goal.", emb[:, -1])
        pp = O.plan_proposal(sd, "plan_proposal.", emb[:, 0], goal)
        pr, seq_feat = R.module_forward(post, emb)
        plan = O.straight_through_sample(pr, db["plan_idx"])
        lp, ls, mu, grip = O.decoder_forward(sd, "action_decoder.", plan, emb, goal, emb_slice=(64, 128))
        acts = O.world_to_tcp_frame(db["actions"].float(), db["robot_obs"].float()).double()      # (targets: the oracle builds float32 frames)
        act = O.decoder_loss(lp, ls, mu, grip, acts)
        total = total + act + O.kl_loss(pp, pr, 0.01, 0.8)
        if "lang" in m and torch.any(db["use_for_aux_lang_loss"]):
            clip = clip + O.clip_auxiliary_loss(sd, seq_feat, goal, db["use_for_aux_lang_loss"])
    return total / len(batch) + 3.0 * clip


def test_eager_step_against_the_oracle_pieces_and_birnnref(dev):
    from tests.test_parity_gpu import TOL, close
    from tests.test_rnn_kernel_gpu import _reference

    seed = 11
    kn.set_compute("fp32")
    m = _model(dev, seed, "discrete")
    loss, grads, _ = _step(m, _batch(dev, seed, "discrete"))
    assert "_hulc_step_node" not in m.__dict__, "fp32 mode runs the eager Functions"

    def ref():
        sd = {k: v.detach().cpu().double().requires_grad_(k.startswith("plan_recognition.")) for k, v in m.state_dict().items()}
        raw = syn.make_batch(seed, B, S)
        ob = {}
        for mod, db in raw.items():
            ob[mod] = dict(rgb_static=db["rgb_obs"]["rgb_static"].double(), rgb_gripper=db["rgb_obs"]["rgb_gripper"].double(),
                           actions=db["actions"].double(), robot_obs=db["state_info"]["robot_obs"].double(), plan_idx=db["plan_idx"])
            if mod == "lang":
                ob[mod].update(lang=db["lang"].double(), use_for_aux_lang_loss=db["use_for_aux_lang_loss"])
        total = _oracle_step(sd, ob)
        total.backward()
        return total.detach(), {k: v.grad for k, v in sd.items() if k.startswith("plan_recognition.")}
    total, gref = _reference(ref)
    t = TOL["fp32"]
    close(loss, total, t["loss"], "total loss")
    assert len(gref) == 18
    for k, g in gref.items():
        if k.endswith("weight_hh_l1_reverse"):
            assert not g.any() and not grads[k].any(), k
            continue
        close(grads[k], g, t["grad"], f"g {k}")
    a, b = grads["plan_recognition.birnn_model.bias_hh_l1_reverse"], grads["plan_recognition.birnn_model.bias_ih_l1_reverse"]
    assert torch.equal(a, b) and a.any()


@pytest.mark.parametrize("dist", DISTS)
def test_step_node_eager_and_replayed_graphs_give_the_same_bits(dev, dist):
    _in_child("same_bits", dist)


def _case_same_bits(dev, dist):
    kn.set_compute("bf16")

    def run(calls, **env):
        with switches.scope(HULC_NO_STEP_NODE=None, **env):
            kn.reset_step_state(dev)
            m = _model(dev, 31, dist)
            batch = _batch(dev, 31, dist)
            out = [_step(m, batch) for _ in range(calls)]
        return m.__dict__["_hulc_step_node"], out

    node_e, eager = run(1, HULC_NO_STEP_GRAPH="1")
    assert node_e.captures == 0 and node_e.eager_steps == 1
    node, graphed = run(4, HULC_NO_STEP_GRAPH=None)
    assert node.disabled is None, node.disabled
    assert node.captures == 1 and node.replays == 2 and node.eager_steps == 2, (node.captures, node.replays, node.eager_steps)
    l0, g0, logs0 = eager[0]
    assert torch.isfinite(l0) and all(g is not None and g.abs().max() > 0 for n, g in g0.items()
                                      if "plan_recognition" in n and not n.endswith("weight_hh_l1_reverse"))
    assert not g0["plan_recognition.birnn_model.weight_hh_l1_reverse"].any()
    for i, (l, g, logs) in enumerate(graphed):
        what = "the step node before capture" if i < 2 else "the replayed graphs"
        assert torch.equal(l, l0), (what, i, float(l), float(l0))
        assert logs.keys() == logs0.keys() and all(torch.equal(logs[k], logs0[k]) for k in logs0), (what, i)
        _same(g, g0, f"{what}, call {i}, against the eager node")


@pytest.mark.parametrize("dist", DISTS)
def test_arena_trainer_capture_and_replay_equal_its_eager_steps(dev, dist):
    _in_child("arena_trainer", dist)


def _case_arena_trainer(dev, dist):
    """the sample is drawn from the device step word (nothing injected), which both trainers walk alike"""
    from hulc2_amd.trainer import ArenaTrainer

    kn.set_compute("bf16")

    def run(captured):
        kn.reset_step_state(dev)
        m = _model(dev, 13, dist)
        tr = ArenaTrainer(m, overlap=False)
        batch = _batch(dev, 13, dist, inject=False)
        if captured:
            tr.capture(batch)                                          # (its two warm-up steps are the eager trainer's first two)
            losses = [float(tr.replay()) for _ in range(3)]
        else:
            losses = [float(tr.step(batch, i)) for i in range(5)][2:]
        torch.cuda.synchronize()
        kn.check_faults(dev)
        out = losses, tr.flat_g.clone(), tr.flat_p.clone()
        tr.close()
        return out

    (l_e, g_e, p_e), (l_c, g_c, p_c) = run(False), run(True)
    assert all(torch.isfinite(torch.tensor(l_e))), l_e
    assert l_c == l_e, (l_c, l_e)
    assert torch.equal(g_c, g_e), "gradient arena after the last step"
    assert torch.equal(p_c, p_e), "parameters after five steps (two warm-up steps + three)"
    assert len(set(l_e)) == len(l_e), "the steps train: different losses"


@pytest.mark.parametrize("dist", DISTS)
def test_validation_step_runs(dev, dist):
    kn.set_compute("bf16")
    m = _model(dev, 11, dist)
    m.eval()
    out = m.validation_step(_batch(dev, 3, dist, inject=False), 0)
    torch.cuda.synchronize()
    kn.check_faults(dev)
    vals = {k: v for k, v in m.logged.items() if k.startswith("val")}
    assert vals and all(torch.isfinite(torch.as_tensor(v).float()).all() for v in vals.values()), vals
    assert out is not None


if __name__ == "__main__":
    globals()["_case_" + sys.argv[1]](torch.device("cuda", 0), sys.argv[2])
