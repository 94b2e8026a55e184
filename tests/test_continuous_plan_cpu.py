"""The continuous latent-plan distribution (conf/model/distribution/continuous.yaml) without a GPU: the reference API of
hulc2/utils/distributions.py:15-60 on CPU tensors, the state_dict contract of a model built from the continuous config, and no CPU fallback
behind the hot-path entry points."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions import Independent, Normal

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from hulc2_amd import param_spec  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402
from hulc2_amd.utils.distributions import ContState, DiscState, Distribution  # noqa: E402

P = 256


@pytest.fixture(scope="module")
def dist():
    return Distribution(dist="continuous", plan_features=P)


def _raw(seed=0, B=3):
    return torch.randn(B, 2 * P, generator=torch.Generator().manual_seed(seed)) * 3.0


def test_constructs_and_builds_the_reference_head(dist):
    assert dist.dist == "continuous" and dist.plan_features == P
    head = dist.build_state(64, P)
    assert isinstance(head, nn.Sequential) and len(head) == 1 and isinstance(head[0], nn.Linear)
    assert (head[0].in_features, head[0].out_features) == (64, 2 * P)
    disc = Distribution(dist="discrete", category_size=32, class_size=32)
    assert disc.build_state(64, 1024)[0].out_features == 1024
    assert isinstance(disc.forward_dist(torch.zeros(2, 1024)), DiscState)


def test_forward_dist_is_the_reference_cont_state(dist):
    x = _raw().requires_grad_()
    st = dist.forward_dist(x)
    mean, var = torch.chunk(x, 2, dim=-1)                     # distributions.py:55-59 written out
    std = F.softplus(var) + 0.0001
    assert isinstance(st, ContState) and isinstance(st, tuple) and len(st) == 2
    assert torch.equal(st.mean, mean) and torch.equal(st.std, std)
    m2, s2 = st                                               # tuple-unpackable
    assert torch.equal(m2, mean) and torch.equal(s2, std) and torch.equal(st[0], mean) and torch.equal(st[1], std)
    assert st.raw is x, "the raw [mean | r] tensor rides along for the fused node"
    assert st.mean._base is x or st.mean.data_ptr() == x.data_ptr(), "mean is a view of the raw tensor"
    (st.mean.sum() + st.std.sum()).backward()                 # the fields are differentiable functions of the head output
    assert x.grad is not None and torch.equal(x.grad[:, :P], torch.ones(3, P)) and torch.allclose(x.grad[:, P:], torch.sigmoid(x.detach()[:, P:]))


def test_get_dist_detach_and_sample(dist):
    x = _raw(1).requires_grad_()
    st = dist.forward_dist(x)
    d = dist.get_dist(st)
    assert isinstance(d, Independent) and isinstance(d.base_dist, Normal) and d.reinterpreted_batch_ndims == 1
    assert torch.equal(d.base_dist.loc, st.mean) and torch.equal(d.base_dist.scale, st.std)
    assert d.event_shape == (P,) and d.batch_shape == (3,)
    # a state built by a caller from its own tensors works the same (the reference's ContState(mean, std))
    d2 = dist.get_dist(ContState(st.mean.detach(), st.std.detach()))
    assert torch.equal(d2.base_dist.loc, st.mean.detach())
    det = dist.detach_state(st)
    assert isinstance(det, ContState) and not det.mean.requires_grad and not det.std.requires_grad
    assert torch.equal(det.mean, st.mean.detach()) and torch.equal(det.std, st.std.detach())
    det2 = dist.detach_state(ContState(st.mean, st.std))
    assert isinstance(det2, ContState) and not det2.mean.requires_grad and torch.equal(det2.std, st.std.detach())
    torch.manual_seed(7)
    plan = dist.sample_latent_plan(d)
    torch.manual_seed(7)
    want = Independent(Normal(st.mean, st.std), 1).sample()   # distributions.py:37-41: not flattened for the continuous plan
    assert plan.shape == (3, P) and torch.equal(plan, want)


def test_model_from_the_continuous_config_keeps_the_state_dict_contract():
    cfg = default_model_config(distribution="continuous")
    assert dict(cfg["distribution"]) == {"_target_": "hulc2.utils.distributions.Distribution", "dist": "continuous", "plan_features": 256}
    m = instantiate(cfg)
    sd = m.state_dict()
    assert tuple(sd["plan_proposal.fc_state.0.weight"].shape) == (512, 2048)
    assert tuple(sd["plan_recognition.fc_state.0.weight"].shape) == (512, 4096)
    lo, hi = m.action_decoder.perceptual_emb_slice
    assert m.action_decoder.rnn.weight_ih_l0.shape[1] == (hi - lo) + 32 + 256
    assert cfg.action_decoder.plan_features == 256 and cfg.plan_proposal.plan_features == 256 and cfg.plan_recognition.plan_features == 256
    want = param_spec.trainable_shapes(plan=2 * 256, decoder_in=(hi - lo) + 32 + 256)
    got = {k: tuple(v.shape) for k, v in m.named_parameters()}
    assert got == {k: tuple(v) for k, v in want.items()}
    # the default is unchanged
    assert dict(default_model_config()["distribution"])["dist"] == "discrete"


def test_hot_path_has_no_cpu_fallback(dist):
    from hulc2_amd.lib import HulcKernelError

    pp, pr = dist.forward_dist(_raw(2)), dist.forward_dist(_raw(3))
    eps = torch.zeros(3, P)
    with pytest.raises(HulcKernelError):
        dist.rsample_plan(pr, seed=1, eps=eps)
    with pytest.raises(HulcKernelError):
        dist.kl_balanced(pp, pr, 0.01, 0.8)
    with pytest.raises(HulcKernelError):
        dist.kl_balanced_segments(pp, pr, 0.01, 0.8, 3)
    with pytest.raises(HulcKernelError):
        dist.rsample_plan_and_kl(pp, pr, 1, None, 0.01, 0.8, 1, eps=eps)
    with pytest.raises(HulcKernelError):                      # a state without the raw head output cannot take the fused path
        dist.kl_balanced(ContState(pp.mean, pp.std), pr, 0.01, 0.8)


def test_new_entry_points_are_declared_and_exported():
    import ctypes

    from hulc2_amd import build, lib

    build.build(verbose=False)
    so = lib.load()
    i, f, u, p = ctypes.c_int, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_void_p
    assert list(so.hulc_gauss_plan_fwd.argtypes) == [p, p, p, u, p, i, i, f, f, i, p, p, p, p, p]
    assert list(so.hulc_gauss_plan_bwd.argtypes) == [p, p, p, u, p, i, i, f, f, f, i, p, p, p, p, p]
    assert so.hulc_abi_version() == 7
