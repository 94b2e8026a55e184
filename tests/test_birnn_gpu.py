"""Module-level GPU tests of the BiRNN posterior (models/plan_encoders/plan_recognition_net.py: PlanRecognitionBiRNNNetwork over
functional.BiRNNPosteriorFn) against tests/birnnref.py at B = 3, S = 5 (H = 2048 is fixed by the reference):

  * fp32 compute, per-step path: the state logits, x and every gradient against the float64 module under the fp32 bars of
    tests/test_parity_gpu.py (activations 1e-4 max-abs over max-abs, gradients 1e-3 relative L2);
  * bf16 compute, the persistent path (paired / solo sweeps) and the per-step path, each under the SAME bars and not against each other:
    outputs with kcheck.compare, gradients with its relative-L2 form, yardstick e_ref = birnnref.module_emulated (every GEMM operand rounded
    to bf16, the state once per wave step, float32 accumulation) against the float64 module, margin 2 as the sweeps have;
  * on every path weight_hh_l1_reverse's gradient is exactly zero and bias_hh_l1_reverse's has the bits of bias_ih_l1_reverse's.
kn.check_faults follows every forward + backward."""
import functools

import pytest
import torch

from tests import birnnref as R
from tests import kcheck as K
from tests.test_parity_gpu import TOL, close
from tests.test_rnn_kernel_gpu import _reference

pytestmark = pytest.mark.gpu

B, S, SEED = 3, 5, 21
MARGIN = 2.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    K.report("tests/test_birnn_gpu.py")


@functools.lru_cache(maxsize=None)
def _case():
    """the seeded case and its references, computed once: float64 module, float32-accumulation bf16 emulation"""
    def build():
        params, emb, g_state, g_x = R.module_case(SEED, B, S)
        ref = R.module_backward(params, emb, g_state, g_x)
        emu = R.module_emulated(params, emb, g_state, g_x, acc=torch.float32, emulate=True)
        return params, emb, g_state, g_x, ref, emu
    return _reference(build)


def _run(dev, compute, persistent):
    """forward + backward of the module on the device -> (state logits, x, {name: gradient} with "emb", whether the persistent path may run)"""
    from hulc2_amd import functional as HF, kernels as kn, switches
    from hulc2_amd.models.plan_encoders.plan_recognition_net import PlanRecognitionBiRNNNetwork
    from hulc2_amd.utils.distributions import Distribution

    params, emb, g_state, g_x, _, _ = _case()
    kn.set_compute(compute)
    try:
        with switches.scope(HULC_NO_RNN_WAVEFRONT=None if persistent else "1"):
            net = PlanRecognitionBiRNNNetwork(128, 1024, 7, 0.0, Distribution(dist="discrete", category_size=32, class_size=32)).to(dev)
            with torch.no_grad():
                for k, v in net.state_dict().items():
                    v.copy_(params[k])
            took = HF._rnn_persistent(B, 2048, dev)
            e = emb.to(dev).requires_grad_(True)
            state, x = net(e)
            logits = state.logit if hasattr(state, "logit") else state[0]
            (logits * g_state.to(dev)).sum().add((x * g_x.to(dev)).sum()).backward()
            torch.cuda.synchronize()
            kn.check_faults(dev)
    finally:
        kn.set_compute("bf16")
    grads = {k: v.grad for k, v in net.named_parameters()}
    grads["emb"] = e.grad
    assert all(g is not None for g in grads.values()), [k for k, g in grads.items() if g is None]
    return logits.detach().view(B, -1), x.detach(), grads, took


def _structure(grads):
    assert not grads["birnn_model.weight_hh_l1_reverse"].any(), "weight_hh_l1_reverse never reaches the output: its gradient is exactly zero"
    assert torch.equal(grads["birnn_model.bias_hh_l1_reverse"], grads["birnn_model.bias_ih_l1_reverse"]), "the reverse biases of layer 1 share their bits"


def test_module_fp32_per_step_against_float64(dev):
    _, _, _, _, (state, x, gref), _ = _case()
    logits, xg, grads, _ = _run(dev, "fp32", False)
    t = TOL["fp32"]
    close(logits, state, t["act"], "state logits")
    close(xg, x, t["act"], "x")
    for k, g in gref.items():
        close(grads[k], g, t["grad"], f"g {k}")
    _structure(grads)


@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "per-step"])
def test_module_bf16_against_the_rounding_emulation(dev, persistent):
    _, _, _, _, (state, x, gref), (state_e, x_e, gemu) = _case()
    logits, xg, grads, took = _run(dev, "bf16", persistent)
    assert took == persistent, "the test must run the path it names (a whole MI355X, nothing sharing it)"
    who = f"birnn {'persistent' if persistent else 'per-step'}"
    K.compare(who, "logits", logits, state, state_e, MARGIN)
    K.compare(who, "x", xg, x, x_e, MARGIN)
    for k, g in gref.items():
        if k == "birnn_model.weight_hh_l1_reverse":
            continue                                                  # exactly zero on both sides: _structure
        K.compare(who, "g " + k.replace("birnn_model.", ""), grads[k], g, gemu[k], MARGIN, grad=True)
    _structure(grads)
