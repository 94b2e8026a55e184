"""The encoder regularisers (dropout_vis_fc, word_dropout_p, l2_normalize_output, l2_normalize_goal_embeddings), the parts that need no GPU:
the placement pinned on the reference (tests/golden/regularisers/encoder_regularisers.npz, tools/gen_regulariser_golden.py), construction and
state_dict of the four modules, the switches that stay unsupported, the mirror's keep fraction, the header and the library's symbols, the
host-side refusals, the configuration helpers and what keys a captured graph."""
import ctypes as c
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from hulc2_amd import lib as L, param_spec  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config, real_world_model_config  # noqa: E402
from oracle import counter_rng as R  # noqa: E402
from tests import regref as G  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "regularisers" / "encoder_regularisers.npz"
ON = dict(dropout_vis_fc=0.1, word_dropout_p=0.1, l2_normalize_output=True, l2_normalize_goal_embeddings=True)


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(FIXTURE, allow_pickle=False))


@pytest.fixture(scope="module")
def sd64():
    names = {k: s for k, s in param_spec.trainable_shapes().items() if k.startswith(tuple(m[0] for m in G.MODULES.values()))}
    return G.state_dict64(names)


# ---- placement, pinned on the reference -------------------------------------------------------------------------------------------------
def test_fixture_carries_its_recipe(fixture):
    assert int(fixture["seed"]) == G.SEED and float(fixture["p"]) == G.P and int(fixture["word"]) == G.WORD
    assert FIXTURE.stat().st_size < 1 << 20
    assert tuple(fixture["static.out"].shape) == (4, 64) and tuple(fixture["gripper.out"].shape) == (4, 64)
    assert tuple(fixture["visual_goal.out"].shape) == (5, 32) and tuple(fixture["language_goal.out"].shape) == (5, 32)
    assert tuple(fixture["static.gx"].shape) == (4, 3, 25, 25) and tuple(fixture["language_goal.gx"].shape) == (5, 384)


@pytest.mark.parametrize("tag", list(G.MODULES))
def test_float64_restatement_reproduces_the_reference(fixture, sd64, tag):
    """tests/regref.py against what the reference's own modules gave with the same masks: float64 on both sides, 1e-9 of each array's norm
    (the two sum in different orders; a mask or a normalisation in another place is off by percents)"""
    got = G.restate(tag, sd64)
    keys = [k for k in fixture if k.startswith(tag + ".")]
    assert sorted(keys) == sorted(got), (keys, sorted(got))
    for k in keys:
        a, b = np.asarray(got[k], dtype=np.float64), fixture[k].astype(np.float64)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        err = np.linalg.norm(a - b) / np.linalg.norm(b)
        assert err < 1e-9, (k, err)


@pytest.mark.parametrize("tag,what", [("static", "mask"), ("gripper", "mask"), ("language_goal", "mask"), ("visual_goal", "l2"), ("static", "l2")])
def test_restatement_notices_a_misplaced_regulariser(fixture, sd64, tag, what):
    """negative control of the pin: the mask shifted by one index, or the normalisation left out, misses the fixture's output by > 1e-4"""
    x, _ = G.inputs(tag)
    keep = G.mask_of(tag, x.shape[0])
    with torch.no_grad():
        if what == "mask":
            y = G.forward(tag, sd64, x, torch.roll(keep.reshape(-1), 1).reshape(keep.shape))
        else:
            y = G.forward(tag, sd64, x, keep, l2=False)
    b = fixture[tag + ".out"]
    assert np.linalg.norm(y.numpy() - b) / np.linalg.norm(b) > 1e-4


def _checkout():
    from oracle import gen_golden
    p = Path(os.environ.get("HULC_REFERENCE", str(gen_golden.REF)))
    return p if (p / "hulc2" / "models" / "encoders" / "goal_encoders.py").is_file() else None


@pytest.mark.skipif(_checkout() is None, reason="no reference checkout on this machine")
def test_generator_check_reproduces_the_fixture():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_regulariser_golden.py"), "--reference", str(_checkout()), "--check"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "identical" in r.stdout, (r.stdout, r.stderr[-2000:])


# ---- the mirror's masks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("site,cols", [(G.STATIC_FC_SITE, 512), (G.GRIPPER_FC_SITE, 512), (G.WORD_DROPOUT_SITE, 384)])
def test_mirror_keep_fraction(p, site, cols):
    keep = G.keep_scales(site, 256, cols, p)
    assert set(np.unique(keep.numpy())) <= {0.0, float(R.keep_scale(p))}
    assert abs(float((keep > 0).double().mean()) - R.keep_probability(p)) < 0.01


def test_sites_are_the_products_and_unused_elsewhere():
    from hulc2_amd.models.encoders import goal_encoders as ge
    from hulc2_amd.models.perceptual_encoders import vision_network as vn
    from hulc2_amd.models.plan_encoders import plan_recognition_net as prn
    assert (vn.STATIC_FC_SITE, vn.GRIPPER_FC_SITE, ge.WORD_DROPOUT_SITE) == (G.STATIC_FC_SITE, G.GRIPPER_FC_SITE, G.WORD_DROPOUT_SITE)
    ours = [vn.STATIC_FC_SITE, vn.GRIPPER_FC_SITE, ge.WORD_DROPOUT_SITE, *vn.STATIC_FC_MODALITY_SITES.values(), *vn.GRIPPER_FC_MODALITY_SITES.values()]
    assert len(set(ours)) == len(ours) == 7
    taken = set(R.trunk_site_ids(prn.TRUNK_SITE)) | {0xA11CE, 0xB0B}
    for s in prn.MODALITY_SITES.values():
        taken |= set(R.trunk_site_ids(s))
    assert not taken & set(ours)
    assert vn.fc_site(1, {"vis": 2, "lang": 3}, None) == 1 and vn.fc_site(1, {"vis": 2, "lang": 3}, "vis") == 2
    assert vn.fc_site(1, {"vis": 2, "lang": 3}, "lang") == 3


# ---- construction ----------------------------------------------------------------------------------------------------------------------------
def _leaf(cfg, **over):
    cfg = dict(cfg)
    cfg.update(over)
    return cfg


def test_the_four_configs_instantiate_with_their_switches_on():
    """(fails on the parent commit: the four constructors raised NotImplementedError)"""
    cfg = default_model_config(**ON)
    pe = cfg["perceptual_encoder"]
    static = instantiate(pe["rgb_static"])
    gripper = instantiate(pe["rgb_gripper"])
    vis = instantiate(_leaf(cfg["visual_goal"], in_features=128))
    lang = instantiate(cfg["language_goal"], lang_net=None)
    for cam in (static, gripper):
        assert isinstance(cam.fc1[2], torch.nn.Dropout) and cam.fc1[2].p == 0.1 and cam.l2_normalize_output is True
        assert cam.drop_p == 0.1
        cam.eval()
        assert cam.drop_p == 0.0                              # nn.Dropout's rule: active iff module.training
    assert vis.l2_normalize_output is True and lang.l2_normalize_output is True
    assert isinstance(lang.mlp[0], torch.nn.Dropout) and lang.mlp[0].p == 0.1


def test_state_dict_keys_and_shapes_equal_the_default_models():
    a = instantiate(default_model_config())
    b = instantiate(default_model_config(**ON))
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[k].shape == sb[k].shape for k in sa)
    assert a.regulariser_key() != b.regulariser_key()
    b.eval()
    assert b.regulariser_key() != a.regulariser_key()        # (the l2 flags hold in eval mode)
    assert b.regulariser_key()[0][0] == 0.0 and b.regulariser_key()[3][0] == 0.0


def test_config_helpers_default_to_the_present_values():
    cfg = default_model_config()
    pe = cfg["perceptual_encoder"]
    for cam in ("rgb_static", "rgb_gripper"):
        assert pe[cam]["dropout_vis_fc"] == 0.0 and pe[cam]["l2_normalize_output"] is False
    assert cfg["visual_goal"]["l2_normalize_goal_embeddings"] is False and cfg["language_goal"]["l2_normalize_goal_embeddings"] is False
    assert cfg["language_goal"]["word_dropout_p"] == 0.0
    rw = real_world_model_config(**ON)
    assert rw["perceptual_encoder"]["rgb_gripper"]["dropout_vis_fc"] == 0.1 and rw["language_goal"]["word_dropout_p"] == 0.1
    assert "dropout_vis_fc" not in rw["perceptual_encoder"]["rgb_static"]          # the R3M trunk has no such switch


def test_unsupported_switches_still_raise():
    cfg = default_model_config()
    pe = cfg["perceptual_encoder"]
    with pytest.raises(NotImplementedError, match="ReLU"):
        instantiate(_leaf(pe["rgb_static"], activation_function="Tanh"))
    with pytest.raises(NotImplementedError, match="sinusoid"):
        instantiate(_leaf(pe["rgb_static"], use_sinusoid=True))
    with pytest.raises(NotImplementedError, match="nature_cnn"):
        instantiate(_leaf(pe["rgb_gripper"], conv_encoder="impala"))
    with pytest.raises(NotImplementedError, match="ReLU"):
        instantiate(_leaf(pe["rgb_gripper"], activation_function="ELU"))
    with pytest.raises(NotImplementedError, match="ReLU"):
        instantiate(_leaf(cfg["visual_goal"], in_features=128, activation_function="Tanh"))
    with pytest.raises(NotImplementedError, match="ReLU"):
        instantiate(_leaf(cfg["language_goal"], activation_function="Tanh"), lang_net=None)
    net = instantiate(_leaf(pe["rgb_static"], spatial_softmax_temp=None))          # a learnable temperature: refused where it would be used
    with pytest.raises(NotImplementedError, match="temperature"):
        net.spatial_softmax(torch.zeros(1, 21, 21, 64))
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            instantiate(_leaf(pe["rgb_static"], dropout_vis_fc=bad))
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            instantiate(_leaf(cfg["language_goal"], word_dropout_p=bad), lang_net=None)


# ---- the header and the library -----------------------------------------------------------------------------------------------------------
NEW = ("hulc_mlp2_rows_fwd_drop", "hulc_mlp2_rows_bwd_drop", "hulc_l2norm_layernorm_fwd_ld", "hulc_l2norm_layernorm_bwd_ld", "hulc_dropout_fwd")


def test_header_declares_and_library_exports_the_symbols():
    protos = L.parse_prototypes((ROOT / "include" / "hulc2_amd.h").read_text())
    so = L.load()
    assert so.hulc_abi_version() == 7
    for name in NEW:
        fn = getattr(so, name)                                   # (AttributeError if the library does not export it)
        assert fn.restype is c.c_int and list(fn.argtypes) == protos[name][1]
    # the library's convention for RNG arguments: float drop_p, unsigned long long seed, const unsigned long long* seed_dev
    for name in ("hulc_mlp2_rows_fwd_drop", "hulc_mlp2_rows_bwd_drop", "hulc_dropout_fwd"):
        assert protos[name][1][-4:] == [c.c_float, c.c_ulonglong, c.c_void_p, c.c_void_p], name


def test_host_side_refusals_need_no_device():
    so = L.load()
    buf = (c.c_float * 4096)()
    a = (c.addressof(buf) + 15) // 16 * 16
    assert so.hulc_dropout_fwd(None, None, 0, 0.1, 1, None, None) == 0, "n == 0 is a successful no-op"
    assert so.hulc_dropout_fwd(None, a, 4, 0.1, 1, None, None) == -1
    for bad in (1.0, -0.5, float("nan")):
        assert so.hulc_dropout_fwd(a, a + 64, 4, bad, 1, None, None) == -2
        assert so.hulc_mlp2_rows_fwd_drop(a, a, a, a, a, None, None, 32, 128, 128, 32, a, bad, 1, None, None) == -2
        assert so.hulc_mlp2_rows_bwd_drop(a, a, a, a, a, a, 32, 128, 128, 32, a, a, a, bad, 1, None, None) == -2
    assert so.hulc_mlp2_rows_fwd_drop(a, a, a, a, a, None, None, 32, 64, 128, 32, a, 0.1, 1, None, None) == -2, "K != 128"
    assert so.hulc_mlp2_rows_fwd_drop(a, a, a, a, a, a, None, 32, 128, 128, 32, a, 0.1, 1, None, None) == -3, "one remainder array"
    assert so.hulc_mlp2_rows_bwd_drop(a, a, a, a, a, a, 32, 128, 128, 32, a, None, a, 0.1, 1, None, None) == -1
    for D, ld in ((0, 8), (257, 300), (64, 63)):
        assert so.hulc_l2norm_layernorm_fwd_ld(a, a, a, 1e-5, 4, D, a, ld, a, a, a, None) == -2
        assert so.hulc_l2norm_layernorm_bwd_ld(a, ld, a, a, a, a, a, 4, D, a, a, a, 0, a, None) == -2
    assert so.hulc_l2norm_layernorm_fwd_ld(a, a, a, 1e-5, 4, 64, a, 64, None, a, a, None) == -1
    assert so.hulc_l2norm_layernorm_bwd_ld(a, 64, a, a, a, a, a, 4, 64, a, a, a, 0, None, None) == -1
