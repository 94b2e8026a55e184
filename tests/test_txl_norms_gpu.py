"""The plan-recognition transformer with encoder_normalize / position_embedding = false on the GPU, from the module up.  The module still
refuses positional_normalize at construction (tests/test_host_cpu.py pins that refusal), so the module-level cases are the four combinations
without it; its stage is tested through functional.transformer_trunk_pooled(pos_norm=...) in (b) and at kernel level in
tests/test_txl_norms_kernel_gpu.py.

  (a) the four constructible combinations against the reference's own evaluation (tests/golden/txl_norms/plan_recognition_norms.npz), on the
      whole-trunk launches and on the per-layer path; the default combination's error on the same path is the yardstick;
  (b) dropout 0.1 on the whole-trunk path against tests/normref.py replaying the device's masks, and the two paths drop the same
      elements of x0;
  (c) who receives gradients: the LayerNorms exactly when their switch is on, never the sinusoid table;
  (d) a Hulc2 with both accepted switches changed through the three training loops (child processes);
  (e) the launch count of a step does not grow.
Relative L2 errors, as tests/test_txl_block_gpu.py."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
pytestmark = pytest.mark.gpu

from hulc2_amd import kernels as kn, switches, synthetic as syn  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402
from tests import normref as N  # noqa: E402
from tests import seqref as Q  # noqa: E402

# (a) error of a combination / error of the default combination on the same path and quantity (a LayerNorm gradient, which the default
# does not have: against the default's larger gradient error).  A LayerNorm renormalises rows that are already of unit scale: it neither
# amplifies nor hides error, so a combination may reach twice the yardstick.  An entry here is an exception with its measured ratio.
RATIO = {}
DEFAULT_RATIO = 2.0
ALL_ON = dict(encoder_normalize=True, position_embedding=False)        # every switch the module accepts, changed from the yaml's value
MODULE_COMBOS = [c for c in N.COMBOS if not c[1]]
LN_NAMES = ("layernorm.weight", "layernorm.bias", "transformer_encoder.norm.weight", "transformer_encoder.norm.bias")
PATHS = {"block": {}, "per_layer": {"HULC_NO_TXL_BLOCK": "1"}}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return np.load(ROOT / N.GOLDEN)


def _rel(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _module(dev, combo, dropout_p=0.0, num_layers=None):
    from hulc2_amd.models.plan_encoders.plan_recognition_net import PlanRecognitionTransformersNetwork
    from hulc2_amd.utils.distributions import Distribution

    kw = dict(N.MODULE_KW, dropout_p=dropout_p)
    if num_layers:
        kw["num_layers"] = num_layers
    m = PlanRecognitionTransformersNetwork(**kw, **dict(zip(N.SWITCHES, combo)), dist=Distribution(**N.DIST_KW))
    N.fill_state_dict_(m.state_dict())
    return m.to(dev)


def _run(m, dev, train: bool, block: bool):
    """forward + backward on the fixture's input and cotangents -> {quantity: tensor} keyed as the fixture"""
    m.train(train)
    m.zero_grad(set_to_none=True)
    emb, c_logits, c_feat = (t.to(dev) for t in N.fixture_inputs())
    emb.requires_grad_(True)
    state, seq_feat = m(emb)
    trunk_node = any(type(fn).__name__.startswith("TxlBlockFn") for fn in _nodes(seq_feat))
    assert trunk_node == block, "the path under test was not taken"
    logits = state.logit.reshape(N.FIX_B, -1)
    ((logits * c_logits).sum() + (seq_feat * c_feat).sum()).backward()
    torch.cuda.synchronize()
    kn.check_faults(dev)
    out = dict(logits=logits.detach(), seq_feat=seq_feat.detach(), d_emb=emb.grad.detach())
    for k, p in m.named_parameters():
        if k in LN_NAMES + ("position_embeddings.weight",) and p.grad is not None:
            out["grad/" + k] = p.grad.detach().clone()
    return out


def _nodes(t):
    """every autograd node behind tensor t"""
    stack, seen = [t.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.append(fn)
        stack += [n for n, _ in fn.next_functions]
    return seen


# ------------------------------------------------------------------------------------------------
# (a) module against fixture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_every_combination_against_the_reference(dev, golden, path):
    kn.set_compute("bf16")
    with switches.scope(**PATHS[path]):
        errs = {}
        for combo in MODULE_COMBOS:
            tag = N.combo_tag(combo)
            m = _module(dev, combo)
            got_eval = _run(m, dev, False, path == "block")
            got_train = _run(m, dev, True, path == "block")
            assert got_eval.keys() == got_train.keys()
            for k in got_eval:
                assert torch.equal(got_eval[k], got_train[k]), f"{tag} {k}: eval and train (dropout_p = 0) differ"
            want = {k[len(tag) + 1:]: golden[k] for k in golden.files if k.startswith(tag + "/") and not k.endswith(("names", "shapes", "pe32"))}
            assert got_eval.keys() == want.keys(), (sorted(got_eval), sorted(want))
            errs[tag] = {k: _rel(got_eval[k], torch.from_numpy(want[k])) for k in want}
    base = errs[N.combo_tag(N.DEFAULT_COMBO)]
    grad_base = max(base["d_emb"], base["grad/position_embeddings.weight"])
    failed = []
    for tag, e in errs.items():
        for k, v in e.items():
            yard = base.get(k, grad_base)
            ratio = v / yard
            print(f"[{path}] {tag} {k:40s} {v:.3e}  default {yard:.3e}  ratio {ratio:.2f}")
            if tag != N.combo_tag(N.DEFAULT_COMBO) and ratio > RATIO.get((path, k), DEFAULT_RATIO):
                failed.append(f"{tag} {k}: {v:.3e} is {ratio:.2f} x the default combination's {yard:.3e}")
    assert base["logits"] < 1.5e-2 and base["seq_feat"] < 1.5e-2, base       # (the yardstick itself is of bf16 class: tests/test_txl_block_gpu.py's bar)
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------------
# (b) dropout
# ------------------------------------------------------------------------------------------------
def _x0_of(seq_feat):
    """layers[0].x as the whole-trunk node saved it (emb, pos, pos_ids, x0, ...)"""
    (node,) = [fn for fn in _nodes(seq_feat) if type(fn).__name__.startswith("TxlBlockFn")]
    return node.saved_tensors[3]


@pytest.mark.parametrize("combo", [(True, False, True), (True, False, False)], ids=N.combo_tag)
def test_dropout_against_the_mask_replaying_reference(dev, combo, monkeypatch):
    """train mode, dropout_p = 0.1, whole-trunk launches with plain bf16 operands, against normref in float64 on the bf16-rounded weights with
    the device's masks replayed.  Bars: tests/test_dropout_gpu.py's — forward quantities 1.5e-2, gradients max(4e-2, 2 e0), e0 = the same
    launches with dropout off against the same reference without masks (the bf16 rounding level of these operands)."""
    from hulc2_amd.models.plan_encoders.plan_recognition_net import TRUNK_SITE

    monkeypatch.setenv("HULC_FP32_SITES", "head")
    kn.set_compute("bf16")
    p, L, FF = 0.1, N.MODULE_KW["num_layers"], N.MODULE_KW["encoder_hidden_size"]
    m = _module(dev, combo, dropout_p=p)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    emb, c_logits, c_feat = N.fixture_inputs()
    keep = Q.trunk_keep(p, TRUNK_SITE, Q.RNG_WORD, N.FIX_B, N.FIX_S, FF, L)
    want = N.module_forward_backward(sd, combo, emb, c_logits, c_feat, keep=keep, bf16_weights=True)
    want0 = N.module_forward_backward(sd, combo, emb, c_logits, c_feat, bf16_weights=True)
    kn.reset_step_state(dev, seed=Q.RNG_WORD)
    got = _run(m, dev, True, True)
    assert int(kn.step_state(dev)[0].item()) == Q.RNG_WORD
    got0 = _run(m, dev, False, True)
    failed = []
    for k in got:
        name = k.replace("grad/", "")
        e, e0 = _rel(got[k], want[name]), _rel(got0[k], want0[name])
        bar = 1.5e-2 if k in ("logits", "seq_feat") else max(4e-2, 2.0 * e0)
        miss = _rel(got[k], want0[name])
        print(f"[dropout {N.combo_tag(combo)}] {k:40s} {e:.3e} (dropout off {e0:.3e}, bar {bar:.3g}; against the reference without masks {miss:.3e})")
        if e > bar:
            failed.append(f"{k}: {e:.3e} > {bar:.3g}")
    assert not failed, "\n".join(failed)
    assert _rel(got["d_emb"], want0["d_emb"]) > 3 * 4e-2, "the reference without masks must miss clearly (a test that cannot fail otherwise)"


def _trunk(m, emb, p, seed, block, table):
    """the trunk WITH the positional LayerNorm, which the module does not take: the whole-trunk launch through the functional layer, or the
    per-layer composition of existing kernels (AddPosFn with p = 0 -> layer_norm -> the pointwise dropout with AddPosFn's seed and element
    index -> the layers -> layer_norm -> SeqMeanFn) -> pooled"""
    from hulc2_amd import functional as HF

    B, S, E = emb.shape
    ids = m._position_ids(S, emb.device)
    layers = [m._layer_params(l) for l in range(m.num_layers)]
    pos_norm = (m.layernorm.weight, m.layernorm.bias)
    enc_norm = (m.transformer_encoder.norm.weight, m.transformer_encoder.norm.bias) if m.encoder_normalize else None
    if block:
        assert HF.txl_block_ok(emb, layers, S, m.num_heads)
        return HF.transformer_trunk_pooled(emb, table, ids, layers, m.num_heads, p, seed, pos_norm, enc_norm)
    x = HF.WordDropoutFn.apply(HF.layer_norm(HF.AddPosFn.apply(emb, table, ids, 0.0, seed, True), *pos_norm), float(p), int(seed)).reshape(B * S, E)
    for l in range(m.num_layers):
        x = HF.transformer_encoder_layer(x, layers[l], B, S, m.num_heads, p, seed + 100 * (l + 1))
    if enc_norm:
        x = HF.layer_norm(x, *enc_norm)
    return HF.SeqMeanFn.apply(x.reshape(B, S, E))


@pytest.mark.parametrize("combo,L", [((True, False, True), 2), ((False, False, False), 2), ((True, False, True), 4)],
                         ids=lambda v: N.combo_tag(v) if isinstance(v, tuple) else f"L{v}")
def test_both_paths_drop_the_same_elements(dev, combo, L, monkeypatch):
    """positional_normalize through the functional layer.  x0 of the whole-trunk launch against AddPosFn(p = 0) -> layer_norm -> dropout of
    the per-layer path under the same seed and device word: zeros at the same places (p = 0.5: half of them), kept values equal to float32
    rounding of two LayerNorm kernels; and pooled and every gradient of both paths agree to tests/test_txl_block_gpu.py's bars (6e-3
    forward, 3e-2 gradients) at p = 0.1.  L = 4 with both LayerNorms makes ten of them: more than one hulc_ln_partial_reduce_multi
    launch takes (8), so the gradients of layer 3's norm2 and of both new LayerNorms come from the second launch of the loop"""
    from hulc2_amd import functional as HF
    from hulc2_amd.models.plan_encoders.plan_recognition_net import TRUNK_SITE

    monkeypatch.setenv("HULC_FP32_SITES", "head")
    kn.set_compute("bf16")
    m = _module(dev, combo, num_layers=L)
    m.train()
    table = m.position_embeddings.weight if combo[2] else m.positional_encoder.table
    kn.reset_step_state(dev, seed=Q.RNG_WORD)
    emb0, _, _ = N.fixture_inputs()
    emb = emb0.to(dev).requires_grad_(True)
    pooled = _trunk(m, emb, 0.5, TRUNK_SITE, True, table)
    x0 = _x0_of(pooled).reshape(N.FIX_B, N.FIX_S, N.E)
    ids = torch.arange(N.FIX_S, device=dev)
    y = HF.WordDropoutFn.apply(HF.layer_norm(HF.AddPosFn.apply(emb, table, ids, 0.0, TRUNK_SITE, True), m.layernorm.weight, m.layernorm.bias), 0.5, int(TRUNK_SITE))
    torch.cuda.synchronize()
    assert torch.equal(x0 == 0, y == 0), "the two paths drop different elements"
    frac = float((x0 == 0).float().mean())
    assert 0.4 < frac < 0.6, frac
    assert float((x0 - y).abs().max()) <= 64 * 2.0 ** -24 * float(y.abs().max()), "kept values: two float32 LayerNorms of the same rows"
    r = torch.randn(N.FIX_B, N.E, generator=torch.Generator().manual_seed(6)).to(dev)
    res = []
    for block in (True, False):
        m.zero_grad(set_to_none=True)
        e = emb0.to(dev).requires_grad_(True)
        kn.reset_step_state(dev, seed=Q.RNG_WORD)
        out = _trunk(m, e, 0.1, TRUNK_SITE, block, table)
        (out * r).sum().backward()
        torch.cuda.synchronize()
        kn.check_faults(dev)
        g = {"pooled": out.detach(), "d_emb": e.grad.detach()}
        g.update({k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
        res.append(g)
    a, b = res
    assert a.keys() == b.keys() and "layernorm.weight" in a and "layernorm.bias" in a
    for k in a:
        e = _rel(a[k], b[k])
        print(f"[paths {N.combo_tag(combo)}] {k:56s} {e:.3e}")
        assert e < (6e-3 if k == "pooled" else 3e-2), (k, e)


# ------------------------------------------------------------------------------------------------
# (c) who receives gradients
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("combo", MODULE_COMBOS, ids=N.combo_tag)
def test_gradients_reach_exactly_the_switched_on_norms(dev, combo, path):
    kn.set_compute("bf16")
    en, pn, pe = combo
    m = _module(dev, combo)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with switches.scope(**PATHS[path]):
        _run(m, dev, True, path == "block")
    named = dict(m.named_parameters())
    for k in ("layernorm.weight", "layernorm.bias"):
        assert (named[k].grad is not None) == pn, k
    for k in ("transformer_encoder.norm.weight", "transformer_encoder.norm.bias"):
        assert (k in named) == en and (not en or named[k].grad is not None), k
    for k in LN_NAMES:
        if k in named and named[k].grad is not None:
            assert float(named[k].grad.abs().max()) > 0 and torch.isfinite(named[k].grad).all(), k
    if pe:
        g = named["position_embeddings.weight"].grad
        assert g is not None and float(g[:N.FIX_S].abs().max()) > 0 and not g[N.FIX_S:].any()
    else:
        assert not any("position" in k for k in named), "the sinusoid table is not a parameter"
        assert "positional_encoder.pe" in dict(m.named_buffers())
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k}: a forward / backward pass wrote to it"


# ------------------------------------------------------------------------------------------------
# (d) the three training loops (child processes), (e) launch count
# ------------------------------------------------------------------------------------------------
def _in_child(case: str) -> None:
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), case], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, f"child `{case}` exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


NEW = ("plan_recognition.transformer_encoder.norm.weight", "plan_recognition.transformer_encoder.norm.bias")


def _model(dev, seed, dropout_p=0.1, **kw):
    m = instantiate(default_model_config(gripper_control=True, dropout_p=dropout_p, **kw)).to(dev)
    syn.fill_state_dict_(m.state_dict(), seed)
    m.train()
    return m


def _loop(dev, steps, seed=43, B=2, S=16):
    """SGD with lr = 0 (the weights never move), dropout 0.1, the plan sample injected -> (model, losses, [{name: .grad} per step])"""
    kn.set_compute("bf16")
    kn.reset_step_state(dev)
    m = _model(dev, seed, **ALL_ON)
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
    torch.cuda.synchronize()
    kn.check_faults(dev)
    return m, losses, grads


def test_step_node_with_norms_on(dev):
    _in_child("step_node")


def _case_step_node(dev):
    """B = 2, S = 16, both accepted switches changed.  The plain autograd loop, the step node run eagerly and its replayed graphs: losses
    bit-identical in all three, every gradient — the two new LayerNorm tensors' among them, present and non-zero — bit-identical between
    the eager and the replayed node"""
    with switches.scope(HULC_NO_STEP_NODE="1"):
        mp, lp, _ = _loop(dev, 6)
    names = [n for n, _ in mp.named_parameters()]
    assert all(n in names for n in NEW) and not any("position" in n for n in names if n.startswith("plan_recognition."))
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
    assert len(set(lg)) == 6, "every step draws fresh masks"
    for i, (a, b) in enumerate(zip(gg, ge)):
        assert a.keys() == b.keys()
        bad = [n for n in a if (a[n] is None) != (b[n] is None) or (a[n] is not None and not torch.equal(a[n], b[n]))]
        assert not bad, f".grad of step {i}: {len(bad)} of {len(a)} tensors differ, e.g. {bad[:3]}"
        for n in NEW:
            assert a[n] is not None and float(a[n].abs().max()) > 0, f"step {i}: {n} received no gradient"
    kn.check_faults(dev)


def test_arena_trainer_with_norms_on(dev):
    _in_child("native_loop")


def _case_native_loop(dev):
    """ArenaTrainer (Adam, lr 2e-4, dropout off) with both accepted switches changed: the new LayerNorm parameters have arena slots and gradient
    sinks; two warm-up steps + three more, eager against
    capture() + three replays: losses and parameters bit for bit; the two new tensors have moved; and they — like every other parameter —
    agree with the reference's loop under hulc2_amd.optim.Adam within the drop-in test's bar (tests/test_optim_dropin_gpu.py:
    2e-6 max(|p|, 1) + 1e-3 lr per tensor)"""
    from hulc2_amd import gradsink
    from hulc2_amd.optim import Adam
    from hulc2_amd.trainer import ArenaTrainer

    LR, seed = 2e-4, 17

    def run(graph):
        kn.set_compute("bf16")
        kn.reset_step_state(dev)
        m = _model(dev, seed, dropout_p=0.0, **ALL_ON)
        init = {n: p.detach().clone() for n, p in m.named_parameters()}
        tr = ArenaTrainer(m, lr=LR, overlap=False)
        batch = syn.make_batch(seed, 2, 16, device=dev)
        if graph:
            tr.capture(batch)
        else:
            for i in range(2):
                tr.step(batch, i)
        losses = [float(tr.replay() if graph else tr.step(batch, 2 + i)) for i in range(3)]
        torch.cuda.synchronize()
        kn.check_faults(dev)
        return m, tr, init, losses

    me, tre, _, le = run(False)
    named = dict(me.named_parameters())
    for n in NEW:
        assert gradsink.get(named[n]) is not None, f"{n} has no gradient sink"
        assert gradsink.written(named[n]), f"{n}: nobody wrote its sink in the last backward"
    pe_flat = tre.flat_p.clone()
    m, tr, init, lg = run(True)
    print(f"[native loop] eager {le}\n[native loop] replay {lg}")
    assert lg == le, (lg, le)
    assert torch.equal(tr.flat_p, pe_flat), "parameters after capture() + 3 replays differ from 5 eager steps"
    now = {n: p.detach().clone() for n, p in m.named_parameters()}
    for n in NEW:
        assert float((now[n] - init[n]).abs().max()) > 0, f"{n} did not move in five Adam steps"
    # the reference's loop: loss.backward(); optimizer.step() with the drop-in Adam
    kn.reset_step_state(dev)
    mo = _model(dev, seed, dropout_p=0.0, **ALL_ON)
    opt = Adam(mo.parameters(), lr=LR)
    batch = syn.make_batch(seed, 2, 16, device=dev)
    for i in range(5):
        opt.zero_grad(set_to_none=True)
        mo.training_step(batch, i).backward()
        opt.step()
    torch.cuda.synchronize()
    kn.check_faults(dev)
    worst_new, worst_other, failed = 0.0, 0.0, []
    for n, p in mo.named_parameters():
        d = float((p.detach() - now[n]).abs().max())
        bar = 2e-6 * max(float(now[n].abs().max()), 1.0) + 1e-3 * LR
        if n in NEW:
            worst_new = max(worst_new, d / bar)
            print(f"[native loop] {n}: max |p_loop - p_replay| {d:.3e} (bar {bar:.3e})")
            if d > bar:
                failed.append(f"{n}: {d:.3e} > {bar:.3e}")
        else:
            worst_other = max(worst_other, d / bar)
    print(f"[native loop] worst difference / bar: new LayerNorm tensors {worst_new:.3f}, every other parameter {worst_other:.3f}")
    assert not failed, "\n".join(failed)


def test_launch_count_does_not_grow(dev):
    _in_child("launch_count")


def _case_launch_count(dev):
    """one eager training step (forward + backward) of the default model and of the model with the encoder's LayerNorm on: the same launches through
    the library, key for key, but for the two trunk launches' names; with the sinusoid table one launch fewer (its batch sum is gone)"""
    def count(**kw):
        kn.set_compute("bf16")
        kn.reset_step_state(dev)
        m = _model(dev, 42, **kw)
        batch = syn.make_batch(42, 2, 16, device=dev)
        with switches.scope(HULC_NO_STEP_NODE="1"):
            for i in range(2):
                m.zero_grad(set_to_none=True)
                m.training_step(batch, i).backward()
            m.zero_grad(set_to_none=True)
            kn.start_timing()
            m.training_step(batch, 2).backward()
            rec = kn.stop_timing()
        kn.check_faults(dev)
        return {k: v[0] for k, v in rec.items()}, {k: v[1] for k, v in rec.items()}

    ren = lambda c: {tuple(str(x).replace("txl_block_norms_", "txl_block_") for x in k): n for k, n in c.items()}
    base, tb = count()
    norms, tn = count(encoder_normalize=True)
    sinus, _ = count(**ALL_ON)
    nb, nn_, ns = sum(base.values()), sum(norms.values()), sum(sinus.values())
    print(f"[launch count] default {nb}, the encoder's LayerNorm on {nn_}, both accepted switches changed {ns}")
    for k in tn:
        if "txl_block" in str(k):
            print(f"[launch count] {k}: {tn[k]:.3f} ms")
    for k in tb:
        if "txl_block" in str(k):
            print(f"[launch count] {k}: {tb[k]:.3f} ms")
    assert any("txl_block_norms_fwd" in str(k) for k in norms) and any("txl_block_norms_bwd" in str(k) for k in norms)
    assert ren(norms) == ren(base), sorted(set(ren(norms).items()) ^ set(ren(base).items()))
    assert ns == nb - 1, (ns, nb)


if __name__ == "__main__":
    assert torch.cuda.is_available()
    globals()["_case_" + sys.argv[1]](torch.device("cuda:0"))
