"""Plan recognition norms without a GPU: the three switches of conf/model/plan_recognition/transformers.yaml (encoder_normalize,
positional_normalize, position_embedding): the four combinations without positional_normalize construct with exactly the reference's
state-dict keys; the four with it are still refused at construction (tests/test_host_cpu.py::test_unsupported_configs_fail_loudly pins that
refusal, so the module keeps it although the stage exists in the kernels).  param_spec and the default config follow all three switches
without changing their defaults, and tests/normref.py — the float64 yardstick of the GPU tests — reproduces
the reference's own outputs and gradients (tests/golden/txl_norms/plan_recognition_norms.npz, tools/gen_txl_norms_golden.py)."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import normref as N
from tests import seqref as Q

ROOT = Path(__file__).resolve().parent.parent
# The fixture is the reference evaluated in float32.  Every value it holds is the end of a chain of dot products, the longest of which has
# 128 terms here (d_model = feed-forward width = 128; the head's 64, the sequence's 7); a float32 dot product of n terms is within n
# half-ulps (n u sum |a_i b_i|, no cancellation assumed) of the exact one.  The bound: 128 float32 half-ulps at the tensor's largest value.
N_RED = 128


@pytest.fixture(scope="module")
def golden():
    return np.load(ROOT / N.GOLDEN)


def _fixture_sd(golden, combo):
    """a state dict with the reference's names and shapes for `combo`, from the fixture alone (no module): zeros, the sinusoid buffer filled"""
    from hulc2_amd.models.plan_encoders.plan_recognition_net import PositionalEncoding

    tag = N.combo_tag(combo) + "/"
    sd = {str(k): torch.zeros([int(v) for v in str(s).split(",")]) for k, s in zip(golden[tag + "names"], golden[tag + "shapes"])}
    if "positional_encoder.pe" in sd:
        sd["positional_encoder.pe"] = PositionalEncoding(N.MODULE_KW["in_features"]).pe.clone()
    return sd


def _module(combo):
    from hulc2_amd.models.plan_encoders.plan_recognition_net import PlanRecognitionTransformersNetwork
    from hulc2_amd.utils.distributions import Distribution

    return PlanRecognitionTransformersNetwork(**N.MODULE_KW, **dict(zip(N.SWITCHES, combo)), dist=Distribution(**N.DIST_KW))


@pytest.mark.parametrize("combo", N.COMBOS, ids=N.combo_tag)
def test_every_combination_constructs_with_the_reference_keys(golden, combo):
    if combo[1]:
        with pytest.raises(NotImplementedError, match="positional_normalize"):
            _module(combo)
        return
    m = _module(combo)
    tag = N.combo_tag(combo) + "/"
    sd = m.state_dict()
    assert sorted(sd) == list(golden[tag + "names"])
    assert [",".join(str(v) for v in sd[k].shape) for k in sorted(sd)] == list(golden[tag + "shapes"])
    en, pn, pe = combo
    assert ("transformer_encoder.norm.weight" in sd) == en
    assert "layernorm.weight" in sd and "layernorm.bias" in sd
    assert ("position_embeddings.weight" in sd) == pe
    names = dict(m.named_parameters())
    if not pe:
        assert tuple(sd["positional_encoder.pe"].shape) == (5000, 1, 128)
        assert not any("position" in k for k in names), "sinusoid mode has no position parameter"
        assert "positional_encoder.pe" in dict(m.named_buffers())


def test_sinusoid_table_equals_the_reference(golden):
    m = _module((False, False, False))
    pe = m.state_dict()["positional_encoder.pe"][:32, 0].double()
    for combo in N.COMBOS:
        if not combo[2]:
            ref = torch.from_numpy(golden[N.combo_tag(combo) + "/pe32"]).double()
            assert (pe - ref).abs().max().item() <= 2.0 ** -23, "sin / cos of float32 arguments"
    assert torch.equal(m.positional_encoder.table, m.positional_encoder.pe[:, 0])
    assert m.positional_encoder.table.data_ptr() == m.positional_encoder.pe.data_ptr()


def bufs_of(param_spec, kw):
    return {k[len("plan_recognition."):]: tuple(s) for k, s in param_spec.buffer_shapes(position_embedding=kw["position_embedding"]).items()
            if k.startswith("plan_recognition.")}


@pytest.mark.parametrize("combo", N.COMBOS, ids=N.combo_tag)
def test_param_spec_follows_the_switches(golden, combo):
    from hulc2_amd import param_spec

    kw = dict(zip(N.SWITCHES, combo))
    spec = {k[len("plan_recognition."):]: tuple(s) for k, s in param_spec.trainable_shapes(
        fc_hidden=N.MODULE_KW["fc_hidden_size"], ff=N.MODULE_KW["encoder_hidden_size"], plan=N.MODULE_KW["plan_features"], **kw).items()
        if k.startswith("plan_recognition.")}
    ref = {k: tuple(v.shape) for k, v in _fixture_sd(golden, combo).items()}            # the reference's own keys for this combination
    assert {**spec, **bufs_of(param_spec, kw)} == ref
    if combo[1]:
        return
    m = _module(combo)
    assert spec == {k: tuple(p.shape) for k, p in m.named_parameters()}
    bufs = bufs_of(param_spec, kw)
    assert bufs == {k: tuple(b.shape) for k, b in m.named_buffers()}


def test_defaults_are_unchanged():
    from hulc2_amd import param_spec
    from hulc2_amd.config import default_model_config

    kw = dict(zip(N.SWITCHES, N.DEFAULT_COMBO))
    assert param_spec.trainable_shapes() == param_spec.trainable_shapes(**kw)
    assert list(param_spec.trainable_shapes()) == list(param_spec.trainable_shapes(**kw))
    spec = param_spec.trainable_shapes()
    assert "plan_recognition.position_embeddings.weight" in spec and "plan_recognition.layernorm.weight" in spec
    assert not any("transformer_encoder.norm." in k or "positional_encoder" in k for k in spec)
    assert param_spec.buffer_shapes() == param_spec.buffer_shapes(position_embedding=True)
    assert not any("plan_recognition" in k for k in param_spec.buffer_shapes())
    cfg, same = default_model_config(), default_model_config(**kw)
    assert cfg == same
    pr = cfg["plan_recognition"]
    assert (pr["encoder_normalize"], pr["positional_normalize"], pr["position_embedding"]) == N.DEFAULT_COMBO
    on = default_model_config(encoder_normalize=True, positional_normalize=True, position_embedding=False)["plan_recognition"]
    assert (on["encoder_normalize"], on["positional_normalize"], on["position_embedding"]) == (True, True, False)
    on.update(encoder_normalize=False, positional_normalize=False, position_embedding=True)
    assert on == pr


@pytest.mark.parametrize("combo", N.COMBOS, ids=N.combo_tag)
def test_normref_reproduces_the_reference(golden, combo):
    tag = N.combo_tag(combo) + "/"
    sd = _fixture_sd(golden, combo)
    N.fill_state_dict_(sd)
    emb, c_logits, c_feat = N.fixture_inputs()
    got = N.module_forward_backward(sd, combo, emb, c_logits, c_feat)
    checked = 0
    for key in golden.files:
        if not key.startswith(tag) or key.endswith(("names", "shapes", "pe32")):
            continue
        ref = torch.from_numpy(golden[key]).double()
        mine = got[key[len(tag):].replace("grad/", "")].reshape(ref.shape)
        err, bound = (mine - ref).abs().max().item(), N.f32_bound(ref, N_RED)
        print(f"[normref] {key:48s} max |diff| {err:.3e}  bound {bound:.3e}")
        assert err <= bound, f"{key}: {err:.3e} > {N_RED} float32 half-ulps at the tensor's largest value ({bound:.3e})"
        checked += 1
    en, pn, pe = combo
    assert checked == 3 + 2 * en + 2 * pn + pe, "the gradients of exactly the LayerNorms that are on, and of the learned table"


@pytest.mark.parametrize("emulate,acc", [(False, torch.float64), (True, torch.float32), (True, torch.float64)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_normref_without_norms_is_seqref_trunk(emulate, acc, p):
    B, S, L, FF = 3, 7, 2, 256
    ops, _, _, _ = Q.trunk_random(B, S, L, FF, 21, p, Q.TRUNK_SITE, Q.RNG_WORD, ops_only=True)
    keep = Q.trunk_keep(p, Q.TRUNK_SITE, Q.RNG_WORD, B, S, FF, L)
    a = Q.trunk(**ops, keep=keep, acc=acc, emulate=emulate)
    b = N.trunk(**ops, keep=keep, acc=acc, emulate=emulate)
    names = [n for n, _ in Q.trunk_tensors(a)]
    assert names == [n for n, _ in N.trunk_tensors(b)], "no tensor of a switched-off stage"
    for (n, x), (_, y) in zip(Q.trunk_tensors(a), N.trunk_tensors(b)):
        assert torch.equal(x, y), f"{n}: normref.trunk without norms differs from seqref.trunk"


def test_normref_stages_sit_where_the_reference_has_them():
    """gamma = 0 makes a LayerNorm the constant beta: x0 = beta * keep (the dropout is behind LN_pos), pooled = beta (LN_enc is ahead of the mean)"""
    B, S, L, FF = 2, 5, 1, 128
    ops, _, _, _ = Q.trunk_random(B, S, L, FF, 3, 0.5, Q.TRUNK_SITE, Q.RNG_WORD, ops_only=True)
    keep = Q.trunk_keep(0.5, Q.TRUNK_SITE, Q.RNG_WORD, B, S, FF, L)
    beta = torch.arange(N.E, dtype=torch.float64) % 7 - 3
    r = N.trunk(**ops, keep=keep, pos_norm=(torch.zeros(N.E, dtype=torch.float64), beta), enc_norm=(torch.zeros(N.E, dtype=torch.float64), beta))
    assert torch.equal(r["x0"], beta[None] * keep["pos"])
    assert torch.equal(r["pooled"], beta[None].expand(B, N.E))
    assert torch.allclose(r["lnpF"][:, 1], ops["dpooled"], rtol=1e-14, atol=0), "dbeta of LN_enc: S tokens of dpooled / S each"
