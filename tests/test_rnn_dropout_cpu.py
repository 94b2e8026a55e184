"""policy_rnn_dropout_p, the parts that need no GPU: construction and what keys a captured graph, the float64 restatement
(tests/rnndropref.py) pinned on torch's own nn.RNN(dropout=p), the header and the library's symbols, the host-side refusals."""
import ctypes as c
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from hulc2_amd import lib as L  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402
from tests import rnndropref as D  # noqa: E402


# ---- construction ----------------------------------------------------------------------------------------------------------------------------
def _model(p):
    cfg = default_model_config()
    cfg["action_decoder"]["policy_rnn_dropout_p"] = p
    return instantiate(cfg)


def test_the_decoder_instantiates_with_rnn_dropout():
    """(fails on the parent commit: the constructor raised NotImplementedError for any value but 0)"""
    m = _model(0.1)
    dec = m.action_decoder
    assert dec.policy_rnn_dropout_p == 0.1 and dec.rnn.dropout == 0.1
    assert dec.rnn_dropout() == (0.1, 0x5EED7001) and dec.rnn_dropout("vis") == (0.1, 0x5EED7101) and dec.rnn_dropout("lang") == (0.1, 0x5EED7201)
    dec.eval()
    assert dec.rnn_dropout("lang") == (0.0, 0x5EED7201)              # nn.RNN's rule: the mask exists iff module.training
    assert list(_model(0.0).state_dict()) == list(m.state_dict())


@pytest.mark.parametrize("bad", [-0.1, 1.0])
def test_probabilities_outside_the_unit_interval_raise(bad):
    cfg = default_model_config()["action_decoder"]
    cfg = dict(cfg, policy_rnn_dropout_p=bad, perceptual_features=128, plan_features=256)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        instantiate(cfg)


def test_the_other_refusals_stay():
    cfg = dict(default_model_config()["action_decoder"], perceptual_features=128, plan_features=256, policy_rnn_dropout_p=0.1)
    for over in (dict(rnn_model="gru_decoder"), dict(num_layers=3), dict(discrete_gripper=False)):
        with pytest.raises(NotImplementedError):
            instantiate(dict(cfg, **over))


def test_regulariser_key_carries_the_effective_probability_last():
    a, b = _model(0.0), _model(0.1)
    assert a.regulariser_key() != b.regulariser_key()
    assert a.regulariser_key()[:-1] == b.regulariser_key()[:-1] and (a.regulariser_key()[-1], b.regulariser_key()[-1]) == (0.0, 0.1)
    a.eval()
    b.eval()
    assert a.regulariser_key() == b.regulariser_key() and b.regulariser_key()[-1] == 0.0
    assert D.DECODER_RNN_SITE == 0x5EED7001 and D.MODALITY_SITES == {"vis": 0x5EED7101, "lang": 0x5EED7201}


# ---- the restatement, pinned on torch's module -------------------------------------------------------------------------------------------------
B, S, I, H, P = 3, 5, 7, 16, 0.5
NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l1", "weight_hh_l1", "bias_ih_l1", "bias_hh_l1")


def _torch_rnn():
    torch.manual_seed(11)
    rnn = torch.nn.RNN(I, H, num_layers=2, nonlinearity="relu", batch_first=True, dropout=P).double()
    x = torch.randn(B, S, I, dtype=torch.float64)
    w = torch.randn(B, S, H, dtype=torch.float64)
    return rnn, x, w


def _grads(out, w, leaves):
    return torch.autograd.grad((out * w).sum(), leaves)


def test_restatement_equals_torch_rnn_in_train_mode():
    rnn, x, w = _torch_rnn()
    rnn.train()
    xa = x.clone().requires_grad_()
    torch.manual_seed(123)
    out, h_n = rnn(xa)
    g_t = _grads(out, w, [xa] + [getattr(rnn, n) for n in NAMES])
    keep = D.torch_mask(123, P, S, B, H)                            # the time-major draw under the same seed
    assert 0 < int((keep == 0).sum()) < keep.numel() and float(keep.max()) == 2.0
    xb = x.clone().requires_grad_()
    params = [getattr(rnn, n).detach().clone().requires_grad_() for n in NAMES]
    h1, hn = D.two_layer_rnn(xb, *params, keep=keep)
    g_r = _grads(h1, w, [xb] + params)
    assert (h1 - out).abs().max().item() <= 1e-12 and (hn - h_n).abs().max().item() <= 1e-12
    for name, a, b in zip(("x",) + NAMES, g_r, g_t):
        assert (a - b).abs().max().item() <= 1e-12, name
    # the batch-major draw is another mask: the restatement fed with it is far from the module
    torch.manual_seed(123)
    other = torch.dropout(torch.ones(B, S, H, dtype=torch.float64), P, True).permute(1, 0, 2)
    assert (D.two_layer_rnn(x, *params, keep=other)[0] - out).abs().max().item() > 1e-3


def test_restatement_equals_torch_rnn_in_eval_mode():
    rnn, x, _ = _torch_rnn()
    rnn.eval()
    out, h_n = rnn(x)
    params = [getattr(rnn, n).detach() for n in NAMES]
    h1, hn = D.two_layer_rnn(x, *params, keep=None)
    assert (h1 - out).abs().max().item() <= 1e-12 and (hn - h_n).abs().max().item() <= 1e-12
    ones = D.keep_scales(0.0, D.DECODER_RNN_SITE, D.RNG_WORD, S, B, H)
    assert torch.equal(D.two_layer_rnn(x, *params, keep=ones)[0], h1)


def test_sweep_with_a_mask_of_ones_is_seqrefs_sweep():
    """the masked sweep restates seqref.rnn_sweep: with p = 0 both modes give its rows bit for bit (small H, random operands)"""
    from tests import seqref as Q
    h, s, b = 32, 3, 2
    g = torch.Generator().manual_seed(5)
    r = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)
    ops = dict(wA=r(h, h), wB1=r(h, h), wB2=r(h, h), add1=r(s, b, h), bias2=(r(h), None), relu=True)
    want = Q.rnn_sweep(s, b, h, **ops)
    for mode in (D.MODE_K, D.MODE_N):
        assert torch.equal(D.sweep(s, b, h, **ops, keep=torch.ones(s, b, h, dtype=torch.float64), mode=mode), want)


def test_sweep_modes_are_forward_and_backward_of_the_restatement():
    """the K-side sweep is two_layer_rnn's forward, the N-side sweep its autograd backward, under one counter-RNG mask (float64, small H)"""
    h, s, b, p = 16, 4, 3, 0.5
    g = torch.Generator().manual_seed(7)
    r = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)
    keep = D.keep_scales(p, D.DECODER_RNN_SITE, D.RNG_WORD, s, b, h)
    w_hh0, w_ih1, w_hh1, b0, b1 = r(h, h) / 4, r(h, h) / 4, r(h, h) / 4, r(h), r(h)
    pre0 = r(s, b, h).requires_grad_()                               # layer 0's input projection, per step
    h0p, h1p, outs, h0s = torch.zeros(b, h, dtype=torch.float64), torch.zeros(b, h, dtype=torch.float64), [], []
    for t in range(s):
        h0p = torch.relu(pre0[t] + h0p @ w_hh0.t() + b0)
        h1p = torch.relu((h0p * keep[t]) @ w_ih1.t() + h1p @ w_hh1.t() + b1)
        h0s.append(h0p)
        outs.append(h1p)
    z = D.sweep(s, b, h, w_hh0, w_ih1, w_hh1, keep, D.MODE_K, add1=pre0.detach(), bias1=(b0, None), bias2=(b1, None), relu=True)
    for t in range(s):
        assert (z[t + 1, :, :h] - h0s[t]).abs().max().item() <= 1e-12 and (z[t + 2, :, h:] - outs[t]).abs().max().item() <= 1e-12
    dH = r(s, b, h)
    (torch.stack(outs) * dH).sum().backward()
    # reversed sweep: wave step tau gates delta1 with h1_{S-1-tau} and delta0 with h0_{S-tau}
    mask1 = torch.stack([outs[s - 1 - tau].detach() for tau in range(s)])
    mask2 = torch.stack([torch.zeros(b, h, dtype=torch.float64)] + [h0s[s - tau].detach() for tau in range(1, s + 1)])
    d = D.sweep(s, b, h, w_hh1.t(), w_ih1.t(), w_hh0.t(), keep, D.MODE_N, add1=dH.flip(0), mask1=mask1, mask2=mask2)
    for tau in range(1, s + 1):                                      # row tau + 1 of the sweep holds delta0_{S - tau} = d loss / d pre0[S - tau]
        assert (d[tau + 1, :, h:] - pre0.grad[s - tau]).abs().max().item() <= 1e-12


# ---- the header and the library -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbols():
    protos = L.parse_prototypes((ROOT / "include" / "hulc2_amd.h").read_text())
    so = L.load()
    assert so.hulc_abi_version() == 7
    for name in ("hulc_rnn_wavefront_drop", "hulc_rnn_drop_rows"):
        fn = getattr(so, name)                                   # (AttributeError if the library does not export it)
        assert fn.restype is c.c_int and list(fn.argtypes) == protos[name][1]
    # the existing sweep and its descriptor are untouched; the mask's values go by value, the RNG triple in the library's order
    assert protos["hulc_rnn_wavefront"][1] == [c.c_void_p] * 3
    assert protos["hulc_rnn_wavefront_drop"][1] == [c.c_void_p, c.c_float, c.c_ulonglong, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p]
    assert protos["hulc_rnn_drop_rows"][1] == [c.c_void_p, c.c_long, c.c_long, c.c_int, c.c_long, c.c_float, c.c_ulonglong, c.c_void_p,
                                               c.c_void_p, c.c_long, c.c_void_p, c.c_long, c.c_void_p]
    assert (L.DEFINES["HULC_RNN_DROP_K"], L.DEFINES["HULC_RNN_DROP_N"]) == (D.MODE_K, D.MODE_N)
    S_, B_ = 32, 64
    assert so.hulc_rnn_wavefront_drop_workspace(S_, B_, 2048) - so.hulc_rnn_wavefront_workspace(S_, B_, 2048) == S_ * B_ * 2048 // 8


def test_host_side_refusals_need_no_device():
    so = L.load()
    buf = (c.c_float * 4096)()
    a = (c.addressof(buf) + 15) // 16 * 16
    assert so.hulc_rnn_drop_rows(None, 0, 0, 96, 0, 0.1, 1, None, None, 0, None, 0, None) == 0, "rows == 0 is a successful no-op"
    assert so.hulc_rnn_drop_rows(a, 96, 2, 96, 0, 0.1, 1, None, None, 0, None, 0, None) == -1
    for bad in (1.0, -0.5, float("nan")):
        assert so.hulc_rnn_drop_rows(a, 96, 2, 96, 0, bad, 1, None, a + 4096, 96, None, 0, None) == -2
    assert so.hulc_rnn_drop_rows(a, 96, 2, 98, 0, 0.1, 1, None, a + 4096, 98, None, 0, None) == -2      # H % 4
    assert so.hulc_rnn_drop_rows(a, 64, 2, 96, 0, 0.1, 1, None, a + 4096, 96, None, 0, None) == -2      # pitch < H
    wave = L.RnnWaveDesc()
    for bad in (1.0, -0.5, float("nan")):
        assert so.hulc_rnn_wavefront_drop(c.byref(wave), bad, 1, None, D.MODE_K, -1, 1, a, None) == -2
        assert b"drop_p must be in [0, 1)" in so.hulc_last_error()
    assert so.hulc_rnn_wavefront_drop(c.byref(wave), 0.1, 1, None, D.MODE_K, -1, 1, a, None) == -1      # (an empty descriptor: null pointers)
