"""CPU tests of the paired recurrent sweep's reference and binding (tests/birnnref.py, hulc_rnn_wavefront_pair): no GPU needed.

  * birnnref.pair_sweep with the decoder sweep's lag put back IS seqref.rnn_sweep with wB1 = 0, bit for bit, in every mode of that reference
    (plain float64, bf16 rounding points with float32 and float64 accumulation, forward and backward operands);
  * one direction of torch's own nn.RNN(relu, bidirectional) layer, forward and reverse, is the paired sweep's two halves with the second
    half's operands walked backwards: the reading of the contract the BiRNN posterior relies on;
  * the lattice builder's cases hold (2^24 condition, f32 == f64 emulation) and the two halves differ, so a swapped half cannot pass;
  * the header declares hulc_rnn_wavefront_pair, the library exports it and kernels.rnn_wavefront_pair exists (fails without the feature)."""
import pytest
import torch

from tests import birnnref as R
from tests import seqref as Q

H = 2048


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("acc,emulate", [(torch.float64, False), (torch.float32, True), (torch.float64, True)], ids=["plain", "emu32", "emu64"])
def test_pair_sweep_with_the_lag_put_back_is_rnn_sweep(backward, acc, emulate):
    S, B = 3, 2
    ops, _, _, _ = Q.rnn_random(S, B, seed=5, backward=backward)
    ops["wB1"] = torch.zeros(H, H, dtype=torch.float64)
    want = Q.rnn_sweep(S, B, H, **ops, acc=acc, emulate=emulate)
    pair = {k: v for k, v in ops.items() if k != "wB1"}
    got = R.pair_sweep(S, B, H, **pair, add2=None, acc=acc, emulate=emulate, lag=True)
    assert got.shape == want.shape == (S + 2, B, 2 * H)
    assert torch.equal(got, want)
    # (backward operands carry no biases: with wB1 = 0 nothing ever enters their second half)
    assert got[1:S + 1, :, :H].any() and (backward or got[2:, :, H:].any())


def test_pair_sweep_is_a_bidirectional_rnn_layer():
    """nn.RNN(relu, bidirectional=True), one layer, float64: forward direction = first half, reverse direction = second half fed its input
    projections from the far end — row tau + 1 of the sweep is [h_fwd at time tau | h_bwd at time S - 1 - tau]"""
    S, B, K, Hs = 4, 3, 8, 16
    g = torch.Generator().manual_seed(3)
    rnn = torch.nn.RNN(K, Hs, num_layers=1, nonlinearity="relu", bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for p in rnn.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3)
        x = torch.randn(B, S, K, generator=g, dtype=torch.float64)
        out, _ = rnn(x)                                                 # (B, S, 2 Hs)
        xt = x.transpose(0, 1)                                          # (S, B, K)
        z = R.pair_sweep(S, B, Hs, rnn.weight_hh_l0, rnn.weight_hh_l0_reverse, add1=xt @ rnn.weight_ih_l0.t(),
                         add2=(xt @ rnn.weight_ih_l0_reverse.t()).flip(0), bias1=(rnn.bias_ih_l0, rnn.bias_hh_l0),
                         bias2=(rnn.bias_ih_l0_reverse, rnn.bias_hh_l0_reverse), relu=True)
    assert not z[0].any()
    torch.testing.assert_close(z[1:, :, :Hs], out[:, :, :Hs].transpose(0, 1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(z[1:, :, Hs:].flip(0), out[:, :, Hs:].transpose(0, 1), rtol=1e-12, atol=1e-12)
    with torch.no_grad():
        solo = R.pair_sweep(S, B, Hs, rnn.weight_hh_l0, None, add1=xt @ rnn.weight_ih_l0.t(), bias1=(rnn.bias_ih_l0, rnn.bias_hh_l0), relu=True)
    assert torch.equal(solo[:, :, :Hs], z[:, :, :Hs]) and not solo[:, :, Hs:].any()


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_pair_lattice_holds_and_its_halves_differ(backward):
    B, S = 7, 3
    ops, want, st = R.pair_lattice_case(B, S, backward)                 # asserts the 2^24 condition and f32 == f64 emulation itself
    assert want.shape == (S + 1, B, 2 * H) and not want[0].any()
    assert st["sum_max"] < Q.EXACT and st["nonzero"] > 0.05, st
    assert not torch.equal(want[1:, :, :H], want[1:, :, H:]) and not torch.equal(want[1:, :, H:], want[1:, :, H:].flip(0))
    assert torch.equal(R.pair_rows(want)[: S * B], want[1:, :, :H].reshape(-1, H))


def test_the_pair_entry_is_declared_exported_and_wrapped():
    from hulc2_amd import kernels, lib

    protos = lib.parse_prototypes(lib._HEADER_TEXT)
    assert "hulc_rnn_wavefront_pair" in protos
    restype, argtypes = protos["hulc_rnn_wavefront_pair"]
    assert len(argtypes) == 12 and callable(kernels.rnn_wavefront_pair)
    so = lib.load()
    assert so.hulc_rnn_wavefront_pair.argtypes == argtypes and so.hulc_abi_version() == 7
    # a refusal needs no GPU: nothing is launched before the checks
    assert so.hulc_rnn_wavefront_pair(None, None, 0, 0, 0, None, 0, 0, None, 0, None, None) == -1
    assert b"hulc_rnn_wavefront_pair: null pointer" in so.hulc_last_error()


# ---- the module -------------------------------------------------------------------------------------------------------------------
def _dist(kind="discrete"):
    from hulc2_amd.utils.distributions import Distribution
    return Distribution(dist=kind, category_size=32, class_size=32)


@pytest.mark.parametrize("kind,plan_features,state_out", [("discrete", 1024, 1024), ("continuous", 256, 512)])
def test_module_has_the_reference_state_dict(kind, plan_features, state_out):
    """the 18 keys of the reference's PlanRecognitionBiRNNNetwork: birnn_model.{weight,bias}_{ih,hh}_l{0,1}{,_reverse} and fc_state.0
    (layer 1 reads both directions: weight_ih_l1 is (2048, 4096)).  Fails without the feature: the class does not exist."""
    from hulc2_amd.models.plan_encoders.plan_recognition_net import PlanRecognitionBiRNNNetwork
    net = PlanRecognitionBiRNNNetwork(in_features=128, plan_features=plan_features, action_space=7, birnn_dropout_p=0.0, dist=_dist(kind))
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == R.module_shapes(128, state_out) and len(got) == 18
    assert got["birnn_model.weight_ih_l1"] == (2048, 4096) and got["fc_state.0.weight"] == (state_out, 4096)
    assert [k for k, _ in net.named_parameters()] == list(got)


def test_unbuilt_recurrent_posteriors_fail_loudly():
    from hulc2_amd.models.plan_encoders import plan_recognition_net as prn
    with pytest.raises(NotImplementedError, match="birnn_dropout_p"):
        prn.PlanRecognitionBiRNNNetwork(128, 1024, 7, 0.1, _dist())
    with pytest.raises(NotImplementedError, match="bilstm.yaml"):
        prn.PlanRecognitionBiLSTMNetwork(in_features=128, plan_features=1024, action_space=7, birnn_dropout_p=0.0, dist=_dist())


def test_reference_path_resolves_to_this_package():
    """under install_as_hulc2() the reference's import path of the class is ours (a fresh interpreter: the aliases are process-wide)"""
    import subprocess
    import sys
    from pathlib import Path
    code = ("import hulc2_amd.compat as c; c.install_as_hulc2(); import importlib; "
            "m = importlib.import_module('hulc2.models.plan_encoders.plan_recognition_net'); "
            "print(m.PlanRecognitionBiRNNNetwork.__module__, m.PlanRecognitionBiLSTMNetwork.__module__)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=Path(__file__).resolve().parent.parent)
    assert r.returncode == 0, r.stderr[-2000:]
    assert all(name.startswith("hulc2_amd.") for name in r.stdout.split()), r.stdout


def test_written_out_backward_is_autograd_and_nn_rnn():
    """birnnref.module_emulated without rounding, in float64, is autograd through the module's forward (module_backward), whose x is
    torch's own nn.RNN(bidirectional) output at the last step; weight_hh_l1_reverse's gradient is exactly zero and the reverse biases of
    layer 1 agree bit for bit.  (Small sizes: the formulas do not depend on them.)"""
    params, emb, g_state, g_x = R.module_case(3, 2, 4, in_features=8, state_out=6, hidden=16)
    state, x, g = R.module_backward(params, emb, g_state, g_x)
    state2, x2, g2 = R.module_emulated(params, emb, g_state, g_x, acc=torch.float64, emulate=False)
    rnn = torch.nn.RNN(8, 16, num_layers=2, nonlinearity="relu", bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for k, v in rnn.named_parameters():
            v.copy_(params["birnn_model." + k])
        out, _ = rnn(emb.double())
    torch.testing.assert_close(x, out[:, -1], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(state2, state, rtol=1e-12, atol=1e-12)
    assert set(g) == set(g2) and len(g) == 19
    for k in g:
        torch.testing.assert_close(g2[k], g[k], rtol=1e-10, atol=1e-12, msg=k)
    for grads in (g, g2):
        assert not grads["birnn_model.weight_hh_l1_reverse"].any()
        assert torch.equal(grads["birnn_model.bias_hh_l1_reverse"], grads["birnn_model.bias_ih_l1_reverse"])
    # the bf16 emulation is close to it and not equal to it (it is a yardstick, not a copy)
    _, x3, _ = R.module_emulated(params, emb, g_state, g_x, acc=torch.float32, emulate=True)
    assert 0 < (x3 - x).abs().max() < 0.05 * x.abs().max()


# ---- the fixture: the reference's own class on the seeded case (tools/gen_birnn_golden.py) --------------------------------------------
def _fixture():
    import numpy as np
    from pathlib import Path
    return dict(np.load(Path(__file__).resolve().parent / "golden" / "birnn" / "plan_recognition_birnn.npz", allow_pickle=False))


def test_module_has_exactly_the_fixtures_names_and_shapes():
    from hulc2_amd.models.plan_encoders.plan_recognition_net import PlanRecognitionBiRNNNetwork
    fx = _fixture()
    want = {str(n): tuple(int(d) for d in s if d) for n, s in zip(fx["names"], fx["shapes"])}
    net = PlanRecognitionBiRNNNetwork(in_features=128, plan_features=1024, action_space=7, birnn_dropout_p=0.0, dist=_dist())
    assert [str(n) for n in fx["names"]] == list(net.state_dict()) and len(want) == 18
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want == R.module_shapes(128, 1024)


def test_float64_module_reproduces_the_reference_fixture():
    """birnnref's float64 module against the reference's float32 run, every stored tensor within normref.f32_bound: n float32 half-ulps at
    the tensor's largest value, n = 4096 (the longest dot product: layer 1's input projection and fc_state).  On the fixture itself:
    weight_hh_l1_reverse's gradient is exactly zero and the two reverse biases of layer 1 carry the same bits."""
    from tests.normref import f32_bound
    fx = _fixture()
    seed, B, S = (int(v) for v in fx["case"])
    rows = [int(r) for r in fx["rows"]]
    params, emb, g_state, g_x = R.module_case(seed, B, S)
    state, x, g = R.module_backward(params, emb, g_state, g_x)
    checked = 0
    for name, ref in [("logits", state), ("x", x)] + [(f"g.{k}", v) for k, v in g.items()]:
        full = ref
        if name.startswith("g.") and ref.dim() == 2 and name != "g.emb":
            ref = ref[rows]
        got = torch.from_numpy(fx[name]).double().reshape(ref.shape)
        bound = f32_bound(full, 4096)
        err = float((got - ref).abs().max())
        assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"
        if name.startswith("g.") and name != "g.emb":
            # the norm covers the rows that are not sampled.  It is an L2 aggregate, so the elements' float32 errors enter as their RMS, not
            # as their worst case: a reduction of n terms carries about sqrt(n) 2^-24 relative (n = 4096: 3.8e-6); 1e-5 relative leaves the
            # forward-and-backward chain its factor, and one wrong row of 2048 (relative weight ~ 1 / 2048 = 5e-4 of the norm squared) misses it
            n_ref, n_fx = float(full.norm()), float(fx["norm." + name[2:]])
            assert abs(n_ref - n_fx) <= 1e-5 * n_ref, f"{name}: L2 norm {n_fx} against {n_ref}"
        checked += 1
    assert checked == 2 + 19
    assert float(fx["norm.birnn_model.weight_hh_l1_reverse"]) == 0.0 and not fx["g.birnn_model.weight_hh_l1_reverse"].any()
    a, b = fx["g.birnn_model.bias_hh_l1_reverse"], fx["g.birnn_model.bias_ih_l1_reverse"]
    assert a.tobytes() == b.tobytes() and a.any()


def test_default_model_config_is_unchanged_and_birnn_instantiates_a_hulc2():
    """the default stays "transformers" and is exactly the dict it was (posterior= changes the plan_recognition node and nothing else);
    posterior="birnn" gives the birnn.yaml target with birnn_dropout_p 0.0 and action_space 7, proj_vis_lang.im_dim stays 4096 (the BiRNN's
    feature width), and the configuration instantiates a Hulc2 around the recurrent posterior, with either distribution"""
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config
    from hulc2_amd.models.plan_encoders.plan_recognition_net import PlanRecognitionBiRNNNetwork

    plain = lambda c: {k: (plain(v) if hasattr(v, "items") else v) for k, v in c.items()}
    base, same, bi = plain(default_model_config()), plain(default_model_config(posterior="transformers")), plain(default_model_config(posterior="birnn"))
    assert base == same
    assert base["plan_recognition"]["_target_"].endswith(".PlanRecognitionTransformersNetwork") and len(base["plan_recognition"]) == 13
    assert bi["plan_recognition"] == {"_target_": "hulc2.models.plan_encoders.plan_recognition_net.PlanRecognitionBiRNNNetwork",
                                      "in_features": None, "plan_features": None, "action_space": 7, "birnn_dropout_p": 0.0}
    assert {k: v for k, v in bi.items() if k != "plan_recognition"} == {k: v for k, v in base.items() if k != "plan_recognition"}
    assert bi["proj_vis_lang"]["im_dim"] == 4096
    with pytest.raises(NotImplementedError):
        default_model_config(posterior="bilstm")
    for dist, width in (("discrete", 1024), ("continuous", 512)):
        m = instantiate(default_model_config(posterior="birnn", distribution=dist))
        assert type(m).__name__ == "Hulc2" and isinstance(m.plan_recognition, PlanRecognitionBiRNNNetwork)
        assert m.plan_recognition.fc_state[0].weight.shape == (width, 4096) and m.plan_recognition.in_features == 128


def test_param_spec_matches_the_module():
    """trainable_shapes(posterior="birnn") lists the 18 tensors in place of the transformer's and equals the instantiated model's parameters;
    the defaults are unchanged"""
    from hulc2_amd import param_spec
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config

    base, bi = param_spec.trainable_shapes(), param_spec.trainable_shapes(posterior="birnn")
    assert base == param_spec.trainable_shapes(posterior="transformers")
    post = {k[len("plan_recognition."):]: v for k, v in bi.items() if k.startswith("plan_recognition.")}
    assert post == R.module_shapes(128, 1024) and len(post) == 18
    assert {k: v for k, v in bi.items() if not k.startswith("plan_recognition.")} == {k: v for k, v in base.items() if not k.startswith("plan_recognition.")}
    m = instantiate(default_model_config(posterior="birnn"))
    assert {k: tuple(v.shape) for k, v in m.named_parameters()} == dict(bi)
    m0 = instantiate(default_model_config())
    assert {k: tuple(v.shape) for k, v in m0.named_parameters()} == dict(base)
    with pytest.raises(NotImplementedError):
        param_spec.trainable_shapes(posterior="bilstm")
