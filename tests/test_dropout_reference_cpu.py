"""The mask-replaying reference of the posterior trunk's dropout, on the CPU (tests/test_dropout_gpu.py compares the kernels with it):
  placement — the oracle's masked trunk equals torch's own float64 nn.Embedding + nn.Dropout + nn.TransformerEncoder in train mode when
              torch.nn.functional.dropout replays the same masks in call order (position add; per layer the attention probabilities,
              dropout1, the feed-forward dropout, dropout2), forward and every gradient;
  mirror    — the host restatement of the counter RNG (oracle/counter_rng.py) keeps the kernels' keep probability and scale, and the masks of
              different sites are uncorrelated; the trunk sites of the product are the ones the mirror maps."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import counter_rng as R  # noqa: E402
from oracle import hulc2_oracle as O  # noqa: E402

WORD = 0x2545F4914F6CDD1D


def _torch_trunk(L, p):
    torch.manual_seed(11)
    layer = torch.nn.TransformerEncoderLayer(128, 8, dim_feedforward=256, dropout=p)
    enc = torch.nn.TransformerEncoder(layer, num_layers=L, norm=None, enable_nested_tensor=False).double()
    pos = torch.nn.Embedding(40, 128).double()
    drop = torch.nn.Dropout(p)
    with torch.no_grad():
        for q in enc.parameters():
            q.copy_(torch.randn_like(q) * (0.1 if q.dim() == 1 else 0.06))
            if q.dim() == 1 and q.numel() == 128:
                q.add_(0.5)
    for m in enc.layers:       # the layer asks for need_weights=False (a fused kernel that drops inside); route it through the explicit
        mha = m.self_attn      # softmax -> dropout(attn weights) -> bmm path of multi_head_attention_forward
        fwd = mha.forward
        mha.forward = lambda *a, _f=fwd, **k: _f(*a, **dict(k, need_weights=True))
    for mod in (enc, pos, drop):
        mod.train()
    return enc, pos, drop


def _replaying_dropout(masks, p):
    """torch.nn.functional.dropout that hands out the given keep-scales in call order (and checks shape and p of every call)"""
    queue = list(masks)

    def dropout(x, p=0.5, training=True, inplace=False, _want=p):
        assert training and abs(p - _want) < 1e-12 and queue, (training, p, len(queue))
        m = queue.pop(0)
        assert tuple(m.shape) == tuple(x.shape), (tuple(m.shape), tuple(x.shape))
        return x * m
    return dropout, queue


def _call_order(masks, B, S, H, L):
    """the keep-scales in torch's call order and layouts: (S, B, E) sequence-major tokens, (B H, S, S) attention weights"""
    tm = lambda a: torch.from_numpy(a).double().permute(1, 0, 2)
    out = [tm(masks[R.POS])]
    for li in range(L):
        m = masks["layers"][li]
        out += [torch.from_numpy(m[R.ATTN]).double().reshape(B * H, S, S), tm(m[R.OUT]), tm(m[R.FFN]), tm(m[R.LIN2])]
    return out


def _oracle_sd(enc, pos):
    sd = {f"transformer_encoder.layers.{li}.{n}": q.detach().clone().requires_grad_(True) for li, m in enumerate(enc.layers)
          for n, q in m.named_parameters()}
    sd["position_embeddings.weight"] = pos.weight.detach().clone().requires_grad_(True)
    return sd


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,S", [(3, 7), (2, 21)])
def test_masked_oracle_places_masks_where_torch_drops(B, S, p, monkeypatch):
    L, H = 2, 8
    enc, pos, drop = _torch_trunk(L, p)
    masks = R.trunk_masks(p, 0x5EED0001, WORD, B, S, FF=256, L=L)
    g = torch.Generator().manual_seed(12)
    emb, r = torch.randn(B, S, 128, generator=g, dtype=torch.float64), torch.randn(B, 128, generator=g, dtype=torch.float64)

    fake, queue = _replaying_dropout(_call_order(masks, B, S, H, L), p)
    monkeypatch.setattr(torch.nn.functional, "dropout", fake)
    x = emb.clone().requires_grad_(True)
    h = drop((x + pos(torch.arange(S)).unsqueeze(0)).permute(1, 0, 2))     # the reference: x = dropout(emb + pos), (S, B, E)
    y = enc(h).permute(1, 0, 2).mean(dim=1)
    (y * r).sum().backward()
    monkeypatch.undo()
    assert not queue, f"{len(queue)} masks were not used"
    want = {f"transformer_encoder.layers.{li}.{n}": q.grad for li, m in enumerate(enc.layers) for n, q in m.named_parameters()}
    want["position_embeddings.weight"] = pos.weight.grad

    sd = _oracle_sd(enc, pos)
    xo = emb.clone().requires_grad_(True)
    yo = O.plan_recognition_trunk(sd, "", xo, masks=masks).mean(dim=1)
    (yo * r).sum().backward()
    assert _rel(yo, y) < 1e-12, _rel(yo, y)
    assert _rel(xo.grad, x.grad) < 1e-12
    for k, v in want.items():
        assert _rel(sd[k].grad, v) < 1e-11, (k, _rel(sd[k].grad, v))

    # the comparison tells placements apart: layer 0's attention mask moved by one index is far outside the agreement above
    shifted = {R.POS: masks[R.POS], "layers": [dict(m) for m in masks["layers"]]}
    a = masks["layers"][0][R.ATTN]
    shifted["layers"][0][R.ATTN] = np.roll(a.reshape(-1), 1).reshape(a.shape)
    assert _rel(O.plan_recognition_trunk(_oracle_sd(enc, pos), "", emb, masks=shifted).mean(dim=1), y.detach()) > 1e-4


def test_masks_none_is_dropout_off():
    enc, pos, _ = _torch_trunk(2, 0.1)
    emb = torch.randn(2, 5, 128, dtype=torch.float64)
    sd = _oracle_sd(enc, pos)
    ones = R.trunk_masks(0.0, 0x5EED0001, WORD, 2, 5, FF=256)
    assert all((m == 1.0).all() for m in [ones[R.POS]] + [v for d in ones["layers"] for v in d.values()])
    assert torch.equal(O.plan_recognition_trunk(sd, "", emb), O.plan_recognition_trunk(sd, "", emb, masks=ones))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mirror_keep_fraction_and_scale(p):
    n = 1 << 21
    s = R.dropout_scale(0x5EED0001 ^ WORD, np.arange(n, dtype=np.uint64), p)
    q = R.keep_probability(p)
    assert q == 1.0 - int(p * 65536) / 65536
    frac = float((s > 0).mean())
    assert abs(frac - q) < 4.0 * np.sqrt(q * (1 - q) / n), (frac, q)
    assert set(np.unique(s).tolist()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}
    # the four elements of one 64-bit draw use its four 16-bit lanes, so neighbours are independent too
    k = (s > 0).reshape(-1, 4)
    for a in range(4):
        for b in range(a + 1, 4):
            c = np.corrcoef(k[:, a], k[:, b])[0, 1]
            assert abs(c) < 4.0 / np.sqrt(k.shape[0]), (a, b, c)


def test_mirror_sites_are_uncorrelated():
    n = 1 << 18
    idx = np.arange(n, dtype=np.uint64)
    sites = R.trunk_site_ids(0x5EED0001) + R.trunk_site_ids(R.MODALITY_SITES["vis"]) + R.trunk_site_ids(R.MODALITY_SITES["lang"])
    keeps = np.stack([(R.dropout_scale(s ^ WORD, idx, 0.5) > 0).astype(np.float64) for s in sites])
    c = np.corrcoef(keeps)
    off = np.abs(c[~np.eye(len(sites), dtype=bool)])
    assert off.max() < 5.0 / np.sqrt(n), off.max()


def test_mirror_uniform_and_draw():
    u = R.uniform01(0xA11CE ^ WORD, np.arange(1 << 16, dtype=np.uint64))
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert abs(float(u.mean()) - 0.5) < 4.0 * np.sqrt(1.0 / 12.0 / u.size)
    # hulc_rand64 is a pure function of seed + idx * golden: the same sum gives the same draw
    assert R.rand64(0x9E3779B97F4A7C15, 0) == R.rand64(0, 1)
    assert R.rand64(7, 3).dtype == np.uint64


def test_trunk_sites_of_the_product_are_the_mirrors():
    from hulc2_amd.models.plan_encoders import plan_recognition_net as PRN

    assert PRN.TRUNK_SITE == R.TRUNK_SITE and PRN.MODALITY_SITES == R.MODALITY_SITES
    assert PRN.trunk_site("vis") == R.MODALITY_SITES["vis"] and PRN.trunk_site("lang") == R.MODALITY_SITES["lang"]
    calls = [R.TRUNK_SITE, R.MODALITY_SITES["vis"], R.MODALITY_SITES["lang"]]
    subs = [set(R.trunk_site_ids(s, L=4)) for s in calls]              # (the block launch takes up to 4 layers)
    for i in range(len(calls)):
        for j in range(i + 1, len(calls)):
            assert not subs[i] & subs[j], (hex(calls[i]), hex(calls[j]))
    assert not set().union(*subs) & {0xA11CE, 0xB0B}                  # nor the plan sampler's sites
