"""policy_rnn_dropout_p on the GPU, module level: functional.DecoderRNNFn and LogisticDecoderRNN with the inter-layer dropout of
nn.RNN(num_layers=2, dropout=p) against tests/rnndropref.py fed the counter-RNG mask the kernels draw (tests/test_rnn_dropout_cpu.py pins
that restatement on torch's own module; tests/test_rnn_dropout_kernel_gpu.py checks the kernels directly).

  (a) DecoderRNNFn with p = 0.1 against float64: h1 and every gradient, the persistent kernel (bf16, H = 2048) and the per-step path (fp32);
  (b) mask pins: with W_ih0 = W_hh0 = W_hh1 = 0, b_hh0 = 1 and W_ih1 = I the module's h1 IS the mask, so the set of dropped (t, b, j) is read
      off exactly: the persistent kernel and the per-step path drop the elements the convention names, stacked / vis / lang calls take their
      own sites, a moved device word gives another mask, eval mode is the p = 0 module bit for bit;
  (c) one Hulc2 step with p = 0.1 through the three loops (child processes, like the other captured-graph tests)."""
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
pytestmark = pytest.mark.gpu

from hulc2_amd import functional as HF, kernels as kn, switches, synthetic as syn  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402
from tests import rnndropref as D  # noqa: E402
from tests.test_parity_gpu import TOL  # noqa: E402

P_DROP = 0.1
NAMES = ("plan", "emb", "goal", "w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _state(dev):
    kn.set_compute("bf16")
    kn.reset_step_state(dev, seed=D.RNG_WORD)
    yield
    kn.set_compute("bf16")
    kn.reset_step_state(dev)


def _word(dev) -> int:
    return int(kn.step_state(dev)[0].item())


# ------------------------------------------------------------------------------------------------
# (a) DecoderRNNFn against the float64 restatement under the replayed mask
# ------------------------------------------------------------------------------------------------
def _case(B, S, H, P, E, G, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: (torch.rand(*s, generator=g) * 2 - 1) * k
    k0, k1 = (P + E + G) ** -0.5, H ** -0.5
    t = [r(B, P), r(B, S, E + 8), r(B, G), r(H, P + E + G, k=k0), r(H, H, k=k1), r(H, k=k1), r(H, k=k1), r(H, H, k=k1), r(H, H, k=k1), r(H, k=k1),
         r(H, k=k1)]
    return t, r(B, S, H)


def _reference(t, w, lo, hi, keep):
    leaves = [x.double().requires_grad_() for x in t]
    plan, emb, goal = leaves[:3]
    S = emb.shape[1]
    x = torch.cat([plan.unsqueeze(1).expand(-1, S, -1), emb[:, :, lo:hi], goal.unsqueeze(1).expand(-1, S, -1)], dim=2)
    h1, _ = D.two_layer_rnn(x, *leaves[3:], keep=keep)
    return h1.detach(), torch.autograd.grad((h1 * w.double()).sum(), leaves)


def _gpu(dev, t, w, lo, hi, p, site):
    leaves = [x.to(dev).requires_grad_() for x in t]
    h1 = HF.DecoderRNNFn.apply(leaves[0], leaves[1], leaves[2], lo, hi, *leaves[3:], False, False, p, site)
    (h1 * w.to(dev)).sum().backward()
    torch.cuda.synchronize()
    kn.check_faults(dev)
    return h1.detach(), [x.grad for x in leaves]


def _close(what, got, want, tol):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all(), what
    if what.startswith("g"):
        err, scale = (got - want).norm().item(), want.norm().item() + 1e-12
    else:
        err, scale = (got - want).abs().max().item(), want.abs().max().item() + 1e-12
    print(f"[rnn dropout] {what:10s} err / scale {err / scale:.3e} (bar {tol:g})")
    assert err <= tol * scale, f"{what}: err {err:.3e} > {tol:g} * scale {scale:.3e} (ratio {err / scale:.2e})"


@pytest.mark.parametrize("mode,B,S,H", [("bf16", 4, 3, 2048), ("bf16", 33, 5, 2048), ("fp32", 3, 4, 64)])
def test_decoder_rnn_with_dropout_matches_mask_replaying_reference(dev, mode, B, S, H):
    """bars: tests/test_parity_gpu.TOL of the compute mode (activations max-abs over max-abs, gradients relative L2)"""
    P, E, G, lo = 64, 64, 32, 4
    kn.set_compute(mode)
    site = D.MODALITY_SITES["vis"]
    t, w = _case(B, S, H, P, E, G, seed=10 * B + S)
    keep = D.keep_scales(P_DROP, site, _word(dev), S, B, H)
    h_ref, g_ref = _reference(t, w, lo, lo + E, keep)
    h, g = _gpu(dev, t, w, lo, lo + E, P_DROP, site)
    _close("h1", h, h_ref, TOL[mode]["act"])
    for name, a, b in zip(NAMES, g, g_ref):
        _close("g_" + name, a, b, TOL[mode]["grad"])
    # the mask matters at these bars: the same call without dropout misses the reference
    h0, _ = _gpu(dev, t, w, lo, lo + E, 0.0, site)
    miss = (h0.double().cpu() - h_ref).abs().max().item() / h_ref.abs().max().item()
    assert miss > 3 * TOL[mode]["act"], miss


# ------------------------------------------------------------------------------------------------
# (b) mask pins on the module
# ------------------------------------------------------------------------------------------------
PB, PS, PH = 8, 3, 2048


def _decoder(dev, p):
    cfg = dict(default_model_config(gripper_control=False)["action_decoder"], perceptual_features=128, plan_features=256, policy_rnn_dropout_p=p)
    return instantiate(cfg).to(dev)


@pytest.fixture(scope="module")
def pin(dev):
    """a decoder whose h1 is the mask itself: h0_t = relu(b_hh0) = 1 everywhere and layer 1 is the identity on its (dropped) input"""
    dec = _decoder(dev, P_DROP)
    with torch.no_grad():
        for prm in dec.rnn.parameters():
            prm.zero_()
        dec.rnn.bias_hh_l0.fill_(1.0)
        dec.rnn.weight_ih_l1.copy_(torch.eye(PH))
    g = torch.Generator().manual_seed(3)
    inputs = [torch.randn(PB, 256, generator=g).to(dev), torch.randn(PB, PS, 128, generator=g).to(dev), torch.randn(PB, 32, generator=g).to(dev)]
    return dec, inputs


def _dropped(dev, dec, inputs, scope=None):
    """(S, B, H) bool: where layer 1's input was zeroed"""
    h1 = dec._rnn(*inputs, modality_scope=scope).detach()
    torch.cuda.synchronize()
    kn.check_faults(dev)
    assert set(h1.unique().tolist()) <= {0.0, float(h1.max())} and 1.10 < float(h1.max()) < 1.12       # 0 or (a rounding of) 1 / 0.9
    return (h1 == 0).permute(1, 0, 2).cpu()


def _named(site, word):
    return D.keep_scales(P_DROP, site, word, PS, PB, PH) == 0


def test_persistent_path_and_fallback_drop_the_elements_the_convention_names(dev, pin):
    dec, inputs = pin
    dec.train()
    want = _named(D.DECODER_RNN_SITE, D.RNG_WORD)
    assert 0.05 < want.double().mean().item() < 0.15
    assert HF._rnn_persistent(PB, PH, dev), "the persistent kernel must take this geometry on a whole MI355X"
    fast = _dropped(dev, dec, inputs)
    with switches.scope(HULC_NO_RNN_WAVEFRONT="1"):
        slow = _dropped(dev, dec, inputs)
    assert torch.equal(fast, want), f"persistent kernel: {int((fast != want).sum())} elements differ from the convention"
    assert torch.equal(slow, want), f"per-step path: {int((slow != want).sum())} elements differ from the convention"


def test_sites_and_the_device_word_select_the_mask(dev, pin):
    dec, inputs = pin
    dec.train()
    masks = {scope: _dropped(dev, dec, inputs, scope) for scope in (None, "vis", "lang")}
    for scope, site in ((None, D.DECODER_RNN_SITE), ("vis", D.MODALITY_SITES["vis"]), ("lang", D.MODALITY_SITES["lang"])):
        assert torch.equal(masks[scope], _named(site, D.RNG_WORD)), scope
    assert not torch.equal(masks["vis"], masks["lang"]) and not torch.equal(masks[None], masks["vis"])
    assert torch.equal(_dropped(dev, dec, inputs, "vis"), masks["vis"]), "the same word draws the same mask"
    kn.advance_step_state(dev, rng=True, step=False)
    moved = _word(dev)
    assert moved != D.RNG_WORD
    again = _dropped(dev, dec, inputs, "vis")
    assert torch.equal(again, _named(D.MODALITY_SITES["vis"], moved)) and not torch.equal(again, masks["vis"])
    # a module in train mode under no_grad drops as well (the inference sweep), with the stacked site
    with torch.no_grad():
        y = dec._head_outputs(*inputs)[1]                              # h_n (2, B, H): layer 1's final state is the mask of the last step
    torch.cuda.synchronize()
    assert torch.equal((y[1] == 0).cpu(), _named(D.DECODER_RNN_SITE, moved)[PS - 1])
    assert bool((y[0] == 1).all()), "h_n of layer 0 is undropped"


def test_eval_mode_is_the_zero_probability_module_bit_for_bit(dev):
    on, off = _decoder(dev, P_DROP), _decoder(dev, 0.0)
    off.load_state_dict(on.state_dict())
    g = torch.Generator().manual_seed(4)
    inputs = [torch.randn(5, 256, generator=g).to(dev), torch.randn(5, 4, 128, generator=g).to(dev), torch.randn(5, 32, generator=g).to(dev)]
    on.eval()
    off.eval()
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            a, b = on(*inputs), off(*inputs)
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    on.train()
    off.train()
    a, b = on(*inputs), off(*inputs)
    torch.cuda.synchronize()
    kn.check_faults(dev)
    assert not torch.equal(a[2], b[2]), "train mode drops"


# ------------------------------------------------------------------------------------------------
# (c) one step through the three loops (child processes)
# ------------------------------------------------------------------------------------------------
def _in_child(case: str) -> None:
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), case], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, f"child `{case}` exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


def _model(dev, seed, p=P_DROP):
    """the trunk's dropout off: a step's loss depends on the device RNG word through the decoder's mask alone"""
    m = instantiate(default_model_config(gripper_control=True, dropout_p=0.0, policy_rnn_dropout_p=p)).to(dev)
    syn.fill_state_dict_(m.state_dict(), seed)
    m.train()
    return m


def _loop(dev, steps, seed=43, B=2, S=16, p=P_DROP):
    """SGD with lr = 0 (the weights never move) -> (model, losses, [{name: .grad} per step])"""
    kn.set_compute("bf16")
    kn.reset_step_state(dev)
    m = _model(dev, seed, p)
    batch = syn.make_batch(seed, B, S, device=dev)
    opt = torch.optim.SGD([q for q in m.parameters() if q.requires_grad], lr=0.0)
    named = list(m.named_parameters())
    losses, grads = [], []
    for i in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = m.training_step(batch, i)
        loss.backward()
        grads.append({n: (None if q.grad is None else q.grad.detach().clone()) for n, q in named})
        opt.step()
        losses.append(float(loss))
    torch.cuda.synchronize()
    kn.check_faults(dev)
    return m, losses, grads


def test_step_node_with_rnn_dropout(dev):
    _in_child("step_node")


def _case_step_node(dev):
    """B = 2 per modality, S = 16, p = 0.1: the step node run eagerly and its replayed graphs see the same device word at every step —
    losses and every gradient bit-identical over 4 steps; the weights never move, so the steps differ through the mask alone"""
    with switches.scope(HULC_NO_STEP_NODE=None, HULC_NO_STEP_GRAPH="1"):
        me, le, ge = _loop(dev, 4)
    assert me.__dict__["_hulc_step_node"].captures == 0
    with switches.scope(HULC_NO_STEP_NODE=None, HULC_NO_STEP_GRAPH=None):
        mg, lg, gg = _loop(dev, 4)
        node = mg.__dict__["_hulc_step_node"]
        assert node.disabled is None, node.disabled
        assert (node.captures, node.eager_steps, node.replays) == (1, 2, 2), (node.captures, node.eager_steps, node.replays)
        print(f"[step node] eager {le}\n[step node] graph {lg}")
        assert lg == le, (le, lg)
        for i, (a, b) in enumerate(zip(gg, ge)):
            assert a.keys() == b.keys()
            bad = [n for n in a if (a[n] is None) != (b[n] is None) or (a[n] is not None and not torch.equal(a[n], b[n]))]
            assert not bad, f".grad of step {i}: {len(bad)} of {len(a)} tensors differ, e.g. {bad[:3]}"
        assert len(set(lg)) == 4, "every step draws a fresh mask; two consecutive replays differ"
        _, loff, _ = _loop(dev, 4, p=0.0)
        assert len(set(loff)) == 1, loff
    kn.check_faults(dev)


def test_arena_trainer_with_rnn_dropout(dev):
    _in_child("native_loop")


def _case_native_loop(dev):
    """ArenaTrainer (SGD, lr = 0) stepping eagerly against a twin that captures and replays: losses and the whole gradient arena after every
    step, bit for bit; consecutive replays differ (fresh masks on a repeated batch); replay() after the model went to eval mode is refused"""
    from hulc2_amd.trainer import ArenaTrainer

    def run(graph):
        kn.set_compute("bf16")
        kn.reset_step_state(dev)
        m = _model(dev, 17)
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
    m.eval()
    with pytest.raises(RuntimeError, match=r"policy_rnn_dropout_p.*capture\(\)"):
        tr.replay()
    m.train()
    tr.replay()
    torch.cuda.synchronize()
    kn.check_faults(dev)


if __name__ == "__main__":
    assert torch.cuda.is_available()
    globals()["_case_" + sys.argv[1]](torch.device("cuda:0"))
