"""Float64 restatement of the plan-recognition trunk WITH its two optional LayerNorms (csrc/txl_block_norms.hip), built from the pieces of
tests/seqref.py:

    pre0 = emb + pos[pos_ids];  x0 = dropout(LN_pos(pre0))          (positional_normalize; without: x0 = dropout(pre0))
    L post-norm layers                                              (seqref.attn_fwd / ffn / ln_bwd / attn_bwd, seqref.trunk's composition)
    pooled = mean_s LN_enc(y2 of the last layer)                    (encoder_normalize; without: the mean of y2)

and the backward of all of it.  `acc` / `emulate` mean what they mean in seqref.trunk; the two new stages are plain `acc` arithmetic — the
kernels have no bf16 rounding point there.  With both stages off every expression is seqref.trunk's, in its order: the results are the same
bits (tests/test_txl_norms_cpu.py).

Also here, shared by tools/gen_txl_norms_golden.py and the tests: the seeded fill of a PlanRecognitionTransformersNetwork's state dict (the
fixture stores no weights), the fixture's inputs and cotangents, and the module's whole forward / backward on top of the trunk."""
import itertools
import math

import torch

from tests import seqref as Q

E = Q.E
NORM_KEPT = ("pre0", "mean0", "rstd0", "meanF", "rstdF")           # what the forward keeps for the new stages (those that are on)
NORM_BWD = ("lnp0", "lnpF")                                         # what backward leaves: the per-sequence {dgamma, dbeta} partials


def ln_fwd(x, gamma, beta, eps):
    mean = x.mean(-1)
    rstd = torch.rsqrt(((x - mean[:, None]) ** 2).mean(-1) + eps)
    return (x - mean[:, None]) * rstd[:, None] * gamma + beta, mean, rstd


def trunk(emb, pos, pos_ids, layers, keep, dpooled, pos_norm=None, enc_norm=None, eps=1e-5, acc=torch.float64, emulate=False, fwd_emulate=None):
    """seqref.trunk's arguments + pos_norm / enc_norm: (gamma, beta) float64 tensors or None.
    -> seqref.trunk's dict + pre0, mean0, rstd0, lnp0 (positional_normalize) and meanF, rstdF, lnpF (encoder_normalize)"""
    fe = emulate if fwd_emulate is None else fwd_emulate
    B, S, _ = emb.shape
    c = lambda t: t.to(acc)
    out = dict(layers=[])
    if pos_norm is not None:
        pre0 = (c(emb) + c(pos)[pos_ids][None]).reshape(B * S, E)
        xn, mean0, rstd0 = ln_fwd(pre0, c(pos_norm[0]), c(pos_norm[1]), eps)
        x = xn * c(keep["pos"])
        out.update(pre0=pre0.double(), mean0=mean0.double(), rstd0=rstd0.double())
    else:
        x = ((c(emb) + c(pos)[pos_ids][None]).reshape(B * S, E) * c(keep["pos"]))
    out["x0"] = x.double()
    kept = []
    for l, k in zip(layers, keep["layers"]):
        fw = Q.attn_fwd(x, l["Wqkv"], l["bqkv"], l["Wo"], l["bo"], l["g1"], l["be1"], eps, B, S, k["attn"], k["ln1"], acc=acc, emulate=fe)
        y1 = c(fw["y"])
        f = Q.ffn(y1, l["W1"], l["b1"], l["W2"], l["b2"], torch.zeros_like(y1), k["ffn"], acc=acc, emulate=fe)["f"]
        pre2 = y1 + c(f) * c(k["ln2"])
        mean2 = pre2.mean(-1)
        rstd2 = torch.rsqrt(((pre2 - mean2[:, None]) ** 2).mean(-1) + eps)
        y2 = (pre2 - mean2[:, None]) * rstd2[:, None] * c(l["g2"]) + c(l["be2"])
        kept.append(dict(x=x, y1=y1, pre1=c(fw["pre"]), mean1=c(fw["mean"]), rstd1=c(fw["rstd"]), ctx=c(fw["ctx"]), y2=y2, pre2=pre2, mean2=mean2, rstd2=rstd2))
        x = y2
    if enc_norm is not None:
        yF, meanF, rstdF = ln_fwd(x, c(enc_norm[0]), c(enc_norm[1]), eps)
        out.update(meanF=meanF.double(), rstdF=rstdF.double())
        out["pooled"] = yF.reshape(B, S, E).mean(1).double()
    else:
        out["pooled"] = x.reshape(B, S, E).mean(1).double()
    dy = (c(dpooled) / S)[:, None, :].expand(B, S, E).reshape(B * S, E)
    if enc_norm is not None:
        dy, lnpF = Q.ln_bwd(dy, x, meanF, rstdF, c(enc_norm[0]), B)
        out["lnpF"] = lnpF.double()
    bwd = [None] * len(layers)
    for li in range(len(layers) - 1, -1, -1):
        l, k, t = layers[li], keep["layers"][li], kept[li]
        dpre2, lnp2 = Q.ln_bwd(dy, t["pre2"], t["mean2"], t["rstd2"], c(l["g2"]), B)
        r = Q.bf if emulate else Q._ident
        fb = Q.ffn(t["y1"], l["W1"], l["b1"], l["W2"], l["b2"], dpre2 * c(k["ln2"]), k["ffn"], acc=acc, emulate=emulate)
        dy1 = dpre2 + c(fb["dx"])
        bw = Q.attn_bwd(t["x"], l["Wqkv"], l["bqkv"], l["Wo"], l["g1"], B, S, k["attn"], k["ln1"], t["pre1"], t["mean1"], t["rstd1"], dy1, acc=acc, emulate=emulate)
        bwd[li] = dict(d_o=bw["d_o"], dqkv=bw["dqkv"], df=r(dpre2 * c(k["ln2"])), h=fb["h"], dh=fb["dh"], lnp1=bw["ln_partial"], lnp2=lnp2)
        dy = c(bw["dx"])
    if pos_norm is not None:
        demb, lnp0 = Q.ln_bwd(dy * c(keep["pos"]), pre0, mean0, rstd0, c(pos_norm[0]), B)
        out["lnp0"] = lnp0.double()
        out["demb"] = demb.reshape(B, S, E).double()
    else:
        out["demb"] = (dy * c(keep["pos"])).reshape(B, S, E).double()
    for t, b in zip(kept, bwd):
        d = {n: t[n].double() for n in Q.TRUNK_KEPT}
        d.update({n: b[n].double() for n in Q.TRUNK_BWD})
        out["layers"].append(d)
    return out


def trunk_tensors(d: dict):
    """seqref.trunk_tensors + the new stages' tensors that are there"""
    yield from Q.trunk_tensors(d)
    for n in NORM_KEPT + NORM_BWD:
        if n in d:
            yield n, d[n]


def random_norm(seed: int):
    """(gamma, beta) at the model's magnitudes, float32 values as float64"""
    g = torch.Generator().manual_seed(seed)
    n = lambda: torch.randn(E, generator=g, dtype=torch.float64)
    return (1 + 0.1 * n()).float().double(), (0.1 * n()).float().double()


def trunk_random(B, S, L, FF, seed, p, site, word, pos_on: bool, enc_on: bool):
    """seqref.trunk_random's operands with the LayerNorms switched on -> (operands incl. pos_norm / enc_norm / keep, plain, emu32)"""
    ops, _, _, _ = Q.trunk_random(B, S, L, FF, seed, p, site, word, ops_only=True)
    ops["pos_norm"] = random_norm(seed + 1000) if pos_on else None
    ops["enc_norm"] = random_norm(seed + 2000) if enc_on else None
    keep = Q.trunk_keep(p, site, word, B, S, FF, L)
    plain = trunk(**ops, keep=keep)
    e32 = trunk(**ops, keep=keep, acc=torch.float32, emulate=True)
    ops["keep"] = keep
    return ops, plain, e32


# ---------------------------------------------------------------------------------------------------------------------------------
# the module-level fixture (tools/gen_txl_norms_golden.py -> tests/golden/txl_norms/plan_recognition_norms.npz)
# ---------------------------------------------------------------------------------------------------------------------------------
MODULE_KW = dict(in_features=128, num_heads=8, num_layers=2, encoder_hidden_size=128, fc_hidden_size=64, dropout_p=0.0, max_position_embeddings=32,
                 plan_features=32, action_space=7)
DIST_KW = dict(dist="discrete", category_size=4, class_size=8)
FIX_B, FIX_S = 3, 7
FILL_SEED, INPUT_SEED = 20240, 20241
SWITCHES = ("encoder_normalize", "positional_normalize", "position_embedding")
COMBOS = list(itertools.product((False, True), repeat=3))           # values of SWITCHES
DEFAULT_COMBO = (False, False, True)                                # conf/model/plan_recognition/transformers.yaml
GOLDEN = "tests/golden/txl_norms/plan_recognition_norms.npz"


def combo_tag(combo) -> str:
    return "".join("ny"[int(v)] for v in combo)                     # e.g. "nny" = the default


@torch.no_grad()
def fill_state_dict_(sd: dict, seed: int = FILL_SEED) -> None:
    """in place, from ONE seeded generator walked in sorted-name order: LayerNorm gains 1 + 0.1 N, their biases 0.1 N, the learned position
    table 0.5 N, weights U(+-1) / sqrt(fan_in), other biases 0.1 U(+-1); the sinusoid buffer `pe` is left as constructed"""
    g = torch.Generator().manual_seed(seed)
    for name in sorted(sd):
        t = sd[name]
        if name.endswith(".pe"):
            continue
        n = torch.randn(t.shape, generator=g, dtype=torch.float64)
        u = torch.rand(t.shape, generator=g, dtype=torch.float64) * 2 - 1
        if "norm" in name:                                           # layernorm.*, norm1.*, norm2.*, transformer_encoder.norm.*
            v = 1 + 0.1 * n if name.endswith("weight") else 0.1 * n
        elif "position_embeddings" in name:
            v = 0.5 * n
        elif t.dim() >= 2:
            v = u / math.sqrt(t.shape[-1])
        else:
            v = 0.1 * u
        t.copy_(v.to(t.dtype))


def fixture_inputs():
    """-> emb (B, S, E), cotangents of logits (B, 32) and of seq_feat (B, 64): float32 values"""
    g = torch.Generator().manual_seed(INPUT_SEED)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
    return n(FIX_B, FIX_S, E), n(FIX_B, MODULE_KW["plan_features"]), n(FIX_B, MODULE_KW["fc_hidden_size"])


def module_operands(sd: dict, combo, bf16_weights: bool = False):
    """a state dict with the reference's names -> trunk operands (float64 of the stored values; bf16_weights: the four matrices of a layer
    rounded to bf16, what the kernels read) + the head's matrices"""
    en, pn, pe = combo
    d = lambda k: sd[k].detach().double().cpu()
    w = (lambda k: Q.bf(d(k))) if bf16_weights else d
    layers = []
    for l in range(MODULE_KW["num_layers"]):
        p = f"transformer_encoder.layers.{l}."
        layers.append(dict(Wqkv=w(p + "self_attn.in_proj_weight"), bqkv=d(p + "self_attn.in_proj_bias"), Wo=w(p + "self_attn.out_proj.weight"),
                           bo=d(p + "self_attn.out_proj.bias"), W1=w(p + "linear1.weight"), b1=d(p + "linear1.bias"), W2=w(p + "linear2.weight"),
                           b2=d(p + "linear2.bias"), g1=d(p + "norm1.weight"), be1=d(p + "norm1.bias"), g2=d(p + "norm2.weight"), be2=d(p + "norm2.bias")))
    pos = d("position_embeddings.weight") if pe else d("positional_encoder.pe")[:, 0]
    return dict(pos=pos, pos_ids=torch.arange(FIX_S), layers=layers, pos_norm=(d("layernorm.weight"), d("layernorm.bias")) if pn else None,
                enc_norm=(d("transformer_encoder.norm.weight"), d("transformer_encoder.norm.bias")) if en else None,
                head=(d("fc.weight"), d("fc.bias"), d("fc_state.0.weight"), d("fc_state.0.bias")))


def module_forward_backward(sd: dict, combo, emb, c_logits, c_feat, keep=None, bf16_weights=False, acc=torch.float64, emulate=False):
    """the whole module in float64 from its state dict: -> dict logits, seq_feat, d_emb and the gradients of layernorm.* /
    transformer_encoder.norm.* / position_embeddings.weight that exist for `combo` (names as in the state dict), + trunk = the trunk's dict"""
    en, pn, pe = combo
    ops = module_operands(sd, combo, bf16_weights)
    Wf, bfc, Ws, bs = ops.pop("head")
    B, S, _ = emb.shape
    FF, L = MODULE_KW["encoder_hidden_size"], MODULE_KW["num_layers"]
    keep = keep or Q.trunk_keep(0.0, 0, 0, B, S, FF, L)
    emb, c_logits, c_feat = emb.double(), c_logits.double(), c_feat.double()
    zero = torch.zeros(B, E, dtype=torch.float64)
    pooled = trunk(emb=emb, keep=keep, dpooled=zero, acc=acc, emulate=emulate, **ops)["pooled"]
    seq_feat = pooled @ Wf.t() + bfc                                # (the mean commutes with fc: DESIGN §3)
    logits = seq_feat @ Ws.t() + bs
    dpooled = (c_feat + c_logits @ Ws) @ Wf
    t = trunk(emb=emb, keep=keep, dpooled=dpooled, acc=acc, emulate=emulate, **ops)
    out = dict(logits=logits, seq_feat=seq_feat, d_emb=t["demb"], trunk=t)
    if pn:
        out["layernorm.weight"], out["layernorm.bias"] = t["lnp0"][:, 0].sum(0), t["lnp0"][:, 1].sum(0)
    if en:
        out["transformer_encoder.norm.weight"], out["transformer_encoder.norm.bias"] = t["lnpF"][:, 0].sum(0), t["lnpF"][:, 1].sum(0)
    if pe:
        g = torch.zeros_like(ops["pos"])
        g[:S] = t["demb"].sum(0)
        out["position_embeddings.weight"] = g
    return out


def f32_bound(ref: torch.Tensor, n_red: int) -> float:
    """n_red float32 half-ulps at the tensor's largest magnitude (kcheck.half_ulp's formula for float32): what a float32 evaluation whose
    longest reduction has n_red terms may differ from the exact value by"""
    _, ex = torch.frexp(ref.detach().double().abs().max().clamp_min(2.0 ** -126))
    return n_red * 2.0 ** (int(ex) - 1 - 24)
