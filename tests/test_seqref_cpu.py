"""tests/seqref.py is what the kernel-level tests of the fused sequence kernels trust; this file is why.  No GPU needed.

  * with rounding disabled the plain references equal torch's own float64 modules and autograd to 1e-12;
  * every lattice builder's float32 emulation equals its float64 emulation bit for bit (asserted inside the builder, with the 2^24
    condition), and the lattices do push hidden values / states through real bf16 roundings;
  * every yardstick of the random GPU cases is finite and non-zero, and the float64-accumulating emulation stays within the GPU files'
    default margin of it: the margin then measures summation order only."""
import pytest
import torch

from tests import seqref as Q
from tests.kcheck import row_errors

MARGIN = 2.0


def _close(a, b, what):
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
    assert err < 1e-12, f"{what}: {err:.3e}"


@pytest.mark.parametrize("T,FF,p", [(5, 128, 0.0), (70, 384, 0.5), (33, 256, 0.1)])
def test_ffn_reference_matches_torch_autograd(T, FF, p):
    g = torch.Generator().manual_seed(T)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    lin1, lin2 = torch.nn.Linear(128, FF).double(), torch.nn.Linear(FF, 128).double()
    with torch.no_grad():
        for t in (lin1.weight, lin1.bias, lin2.weight, lin2.bias):
            t.copy_(r(*t.shape) * 0.1)
    x, df = r(T, 128).requires_grad_(True), r(T, 128)
    keep = Q.ffn_keep(p, 99, Q.RNG_WORD, T, FF)
    assert p == 0.0 or (0 < (keep == 0).double().mean() < 1)
    h = torch.relu(lin1(x)) * keep
    h.retain_grad()
    f = lin2(h)
    f.backward(df)
    got = Q.ffn(x.detach(), lin1.weight.detach(), lin1.bias.detach(), lin2.weight.detach(), lin2.bias.detach(), df, keep)
    for name, want in (("f", f.detach()), ("dx", x.grad), ("dW1", lin1.weight.grad), ("db1", lin1.bias.grad), ("dW2", lin2.weight.grad), ("h", h.detach())):
        _close(got[name], want, f"ffn {name}")
    _close(got["f_slab"].sum(0), f.detach(), "f slice partials")
    _close(got["dx_slab"].sum(0), x.grad, "dx slice partials")
    _close(got["f_slab"][1:].sum(0) + got["f_slab"][0], f.detach(), "f slice partials")
    if FF > 128:                                        # b2 rides in slice 0 only
        _close(got["f_slab"][1], h.detach()[:, 128:256] @ lin2.weight.detach()[:, 128:256].t(), "f slice 1 carries no bias")


def _rnn_and_operands(S, B, H, seed):
    g = torch.Generator().manual_seed(seed)
    rnn = torch.nn.RNN(H, H, num_layers=2, nonlinearity="relu", batch_first=True).double()
    with torch.no_grad():
        for t in rnn.parameters():
            t.copy_((torch.rand(*t.shape, generator=g, dtype=torch.float64) * 2 - 1) * 0.6)
    x = torch.randn(B, S, H, generator=g, dtype=torch.float64).requires_grad_(True)
    return rnn, x, g


@pytest.mark.parametrize("S,B", [(1, 1), (2, 3), (6, 4)])
def test_rnn_reference_matches_torch_rnn_forward_and_backward(S, B):
    """row r of the sweep is [h0_{r-1} | h1_{r-2}] (the convention of _decoder_rnn_forward); the reversed sweep on the stored activations
    is nn.RNN's autograd backward: row r = [delta1_{S-r} | delta0_{S+1-r}]"""
    H = 8
    rnn, x, g = _rnn_and_operands(S, B, H, 10 * S + B)
    out, hn = rnn(x)
    pre0 = (x.detach() @ rnn.weight_ih_l0.detach().t()).transpose(0, 1).contiguous()            # (S, B, H): the layer-0 input projection
    z = Q.rnn_sweep(S, B, H, rnn.weight_hh_l0.detach(), rnn.weight_ih_l1.detach(), rnn.weight_hh_l1.detach(), add1=pre0,
                    bias1=(rnn.bias_ih_l0.detach(), rnn.bias_hh_l0.detach()), bias2=(rnn.bias_ih_l1.detach(), rnn.bias_hh_l1.detach()), relu=True)
    assert not z[0].any() and not z[1, :, H:].any() and not z[S + 1, :, :H].any()
    _close(z[2:S + 2, :, H:].transpose(0, 1), out.detach(), "h1")
    _close(z[S, :, :H], hn[0].detach(), "h0 final")
    _close(z[S + 1, :, H:], hn[1].detach(), "h1 final")
    # the same with the constant term split off into add1c and only one bias of each pair
    c = torch.randn(B, H, generator=g, dtype=torch.float64)
    z2 = Q.rnn_sweep(S, B, H, rnn.weight_hh_l0.detach(), rnn.weight_ih_l1.detach(), rnn.weight_hh_l1.detach(), add1=pre0 - c, add1c=c,
                     bias1=(rnn.bias_ih_l0.detach() + rnn.bias_hh_l0.detach(), None), bias2=(None, rnn.bias_ih_l1.detach() + rnn.bias_hh_l1.detach()), relu=True)
    _close(z2, z, "add1c / single biases")
    # backward: gradient g1 on every h1_t
    g1 = torch.randn(B, S, H, generator=g, dtype=torch.float64)
    out.backward(g1)
    h0, h1 = z[1:S + 1, :, :H], z[2:S + 2, :, H:]                                               # (S, B, H) by time
    mask1 = h1.flip(0)                                                                          # mask1[tau] = h1_{S-1-tau}
    mask2 = torch.cat([torch.zeros(1, B, H, dtype=torch.float64), h0.flip(0)], 0)               # mask2[tau] = h0_{S-tau}, tau >= 1
    d = Q.rnn_sweep(S, B, H, rnn.weight_hh_l1.detach().t(), rnn.weight_ih_l1.detach().t(), rnn.weight_hh_l0.detach().t(),
                    add1=g1.transpose(0, 1).flip(0).contiguous(), mask1=mask1, mask2=mask2)
    delta0 = d[2:S + 2, :, H:].flip(0)                                                          # (S, B, H) by time
    delta1 = d[1:S + 1, :, :H].flip(0)
    _close((delta0 @ rnn.weight_ih_l0.detach()).transpose(0, 1), x.grad, "dx")
    _close(delta0.sum((0, 1)), rnn.bias_ih_l0.grad, "db0")
    _close(delta1.sum((0, 1)), rnn.bias_hh_l1.grad, "db1")
    _close(torch.einsum("sbn,sbk->nk", delta1, h0), rnn.weight_ih_l1.grad, "dW_ih1")


def test_ffn_lattices_are_exact_and_reach_the_bf16_roundings():
    rounded = ties = 0
    for T in Q.FFN_LATTICE_T:
        for FF in Q.FFN_LATTICE_FF:
            for p in (0.0, 0.5):
                _, want, st = Q.ffn_lattice_case(T, FF, p)           # asserts 2^24 and float32 == float64 inside
                assert all(torch.equal(v, v.float().double()) for v in want.values())
                rounded += st["rounded"]
                ties += st["ties"]
                if T >= 63:
                    assert st["h_max"] > 256, f"T {T} FF {FF} p {p}: the hidden values stay below 256"
    assert rounded > 1000 and ties > 100, f"bf16 roundings of the hidden activation exercised: {rounded}, exact ties: {ties}"


@pytest.mark.parametrize("backward", [False, True])
def test_rnn_lattices_are_exact_and_reach_the_bf16_roundings(backward):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    rounded = ties = 0
    for B, S in Q.RNN_LATTICE_CASES:
        _, want, st = Q.rnn_lattice_case(B, S, backward)              # asserts 2^24 and float32 == float64 inside
        assert torch.equal(want, want.float().double())
        rounded += st["rounded"]
        ties += st["ties"]
        if S == 8:
            assert st["z_max"] > 256 and 0.2 < st["nonzero"] < 0.8, f"B {B} S {S}: {st}"
    assert rounded > 1000 and ties > 100, f"bf16 roundings of the state exercised: {rounded}, exact ties: {ties}"


def _yardsticks(pairs, what, cap=0.05):
    for name, plain, e32, e64 in pairs:
        assert torch.isfinite(plain).all() and torch.isfinite(e32).all()
        e_ref = row_errors(e32, plain).max().item()
        e_64 = row_errors(e64, plain).max().item()
        print(f"[seqref] {what} {name}: e_ref {e_ref:.3e}  float64-accumulating emulation {e_64 / e_ref:.3f} x")
        assert 0.0 < e_ref < cap, f"{what} {name}: yardstick {e_ref}"
        assert e_64 <= MARGIN * e_ref, f"{what} {name}: the rounding points alone score {e_64 / e_ref:.2f} x the yardstick"


@pytest.mark.parametrize("T,FF,p", Q.FFN_RANDOM_CASES)
def test_ffn_yardsticks(T, FF, p):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    _, plain, e32, e64 = Q.ffn_random_case(T, FF, p)
    names = ("f", "dx", "dW1", "db1", "dW2", "f_slab", "dx_slab")
    _yardsticks([(n, Q.ffn_rows(n, plain[n]), Q.ffn_rows(n, e32[n]), Q.ffn_rows(n, e64[n])) for n in names], f"ffn T {T} FF {FF} p {p}")


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("B,S", Q.RNN_RANDOM_CASES)
def test_rnn_yardsticks(B, S, backward):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    _, plain, e32, e64 = Q.rnn_random_case(B, S, backward)
    _yardsticks([("rows", Q.rnn_rows(plain, S), Q.rnn_rows(e32, S), Q.rnn_rows(e64, S))], f"rnn B {B} S {S} {'bwd' if backward else 'fwd'}")


# ------------------------------------------------------------------------------------------------
# attention half
# ------------------------------------------------------------------------------------------------
def _layer_norm(x, gamma, beta, eps):
    mean = x.mean(-1)
    rstd = torch.rsqrt(((x - mean[:, None]) ** 2).mean(-1) + eps)
    return (x - mean[:, None]) * rstd[:, None] * gamma + beta, mean, rstd


@pytest.mark.parametrize("B,S,FF", [(1, 1, 128), (3, 7, 256), (2, 32, 384)])
def test_layer_reference_matches_torch_encoder_layer(B, S, FF):
    """attention half + feed-forward block + LayerNorm2 composed as the post-norm layer, against nn.TransformerEncoderLayer in float64:
    the output, the input gradient and every parameter gradient as the kernels' operands give them (dWqkv = dqkv^T x, dWo = d_o^T ctx, bias
    gradients = row sums, LayerNorm gradients = the per-sequence partials summed)"""
    torch.manual_seed(100 * B + S)
    m = torch.nn.TransformerEncoderLayer(Q.E, Q.NH, dim_feedforward=FF, dropout=0.0, batch_first=True).double()
    with torch.no_grad():
        for q in m.parameters():
            if q.dim() == 1:
                q.add_(torch.randn_like(q) * 0.1)
    x = torch.randn(B, S, Q.E, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B * S, Q.E, dtype=torch.float64)
    y2 = m(x).reshape(B * S, Q.E)
    y2.backward(dy)
    a, d = m.self_attn, lambda t: t.detach()
    xt = d(x).reshape(B * S, Q.E)
    ka, kl = Q.attn_keep(0.0, 0, 0, 0, B, S)
    fw = Q.attn_fwd(xt, d(a.in_proj_weight), d(a.in_proj_bias), d(a.out_proj.weight), d(a.out_proj.bias), d(m.norm1.weight), d(m.norm1.bias),
                    m.norm1.eps, B, S, ka, kl)
    keep = torch.ones(B * S, FF, dtype=torch.float64)
    f = Q.ffn(fw["y"], d(m.linear1.weight), d(m.linear1.bias), d(m.linear2.weight), d(m.linear2.bias), torch.zeros_like(dy), keep)["f"]
    got_y2, mean2, rstd2 = _layer_norm(fw["y"] + f, d(m.norm2.weight), d(m.norm2.bias), m.norm2.eps)
    _close(got_y2, d(y2), "y2")
    dpre2, part2 = Q.ln_bwd(dy, fw["y"] + f, mean2, rstd2, d(m.norm2.weight), B)
    fb = Q.ffn(fw["y"], d(m.linear1.weight), d(m.linear1.bias), d(m.linear2.weight), d(m.linear2.bias), dpre2, keep)
    ns = FF // 128
    bw = Q.attn_bwd(xt, d(a.in_proj_weight), d(a.in_proj_bias), d(a.out_proj.weight), d(m.norm1.weight), B, S, ka, kl, fw["pre"], fw["mean"], fw["rstd"],
                    dpre2, slabs=fb["dx_slab"])                         # dy1 = the residual path + the feed-forward block's slice partials
    assert fb["dx_slab"].shape[0] == ns
    _close(bw["dx"], x.grad.reshape(B * S, Q.E), "dx")
    _close(bw["dqkv"].t() @ xt, a.in_proj_weight.grad, "dWqkv")
    _close(bw["dqkv"].sum(0), a.in_proj_bias.grad, "dbqkv")
    _close(bw["d_o"].t() @ fw["ctx"], a.out_proj.weight.grad, "dWo")
    _close(bw["d_o"].sum(0), a.out_proj.bias.grad, "dbo")
    _close(bw["ln_partial"].sum(0)[0], m.norm1.weight.grad, "dgamma1")
    _close(bw["ln_partial"].sum(0)[1], m.norm1.bias.grad, "dbeta1")
    _close(part2.sum(0)[0], m.norm2.weight.grad, "dgamma2")
    _close(fb["dW1"], m.linear1.weight.grad, "dW1")
    _close(fb["dW2"], m.linear2.weight.grad, "dW2")
    _close(fb["db1"], m.linear1.bias.grad, "db1")


@pytest.mark.parametrize("B,S,n_slab", [(2, 5, 0), (3, 32, 3)])
def test_attention_backward_matches_autograd_under_dropout(B, S, n_slab):
    """the hand-written backward against autograd of the plain forward, with both dropout masks in place"""
    ops, bops, plain, _, _ = Q.attn_random(B, S, seed=B + S, p=0.3, seeds=Q.ATTN_SEEDS, word=Q.RNG_WORD, n_slab=n_slab)
    assert 0 < (ops["keep_attn"] == 0).double().mean() < 1 and 0 < (ops["keep_ln"] == 0).double().mean() < 1
    leaves = {k: ops[k].clone().requires_grad_(True) for k in ("x", "Wqkv", "bqkv", "Wo", "bo", "gamma", "beta")}
    fw = Q.attn_fwd(**{**ops, **leaves})
    dy = bops["dy"] + bops["slabs"].sum(0)
    fw["y"].backward(dy)
    bw = Q.attn_bwd(ops["x"], ops["Wqkv"], ops["bqkv"], ops["Wo"], ops["gamma"], B, S, ops["keep_attn"], ops["keep_ln"],
                    fw["pre"].detach(), fw["mean"].detach(), fw["rstd"].detach(), bops["dy"], slabs=bops["slabs"])
    _close(bw["dx"], leaves["x"].grad, "dx")
    _close(bw["dqkv"].t() @ ops["x"], leaves["Wqkv"].grad, "dWqkv")
    _close(bw["dqkv"].sum(0), leaves["bqkv"].grad, "dbqkv")
    _close(bw["d_o"].t() @ fw["ctx"].detach(), leaves["Wo"].grad, "dWo")
    _close(bw["d_o"].sum(0), leaves["bo"].grad, "dbo")
    _close(bw["ln_partial"].sum(0)[0], leaves["gamma"].grad, "dgamma")
    _close(bw["ln_partial"].sum(0)[1], leaves["beta"].grad, "dbeta")


def test_attention_lattices_are_exact():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    big = dq = 0
    slabs = set()
    for kind, B, S in Q.ATTN_LATTICE_CASES:
        for p in (0.0, 0.5):
            n = Q.attn_lattice_slabs(B, S, p)
            _, fw, _, bw, st = Q.attn_lattice_case(kind, B, S, p, n)  # asserts 2^24, float32 == float64 and the exact probabilities inside
            if bw is not None:
                slabs.add(n)
            big += st["ctx_max"] > 256
            dq += st.get("dq_nonzero", 0)
    assert slabs == set(Q.ATTN_SLABS), f"slab counts of the exact backward cases: {sorted(slabs)}"
    assert big >= 5 and dq > 1000, f"cases with |ctx| above 256: {big}; non-zero dq elements (uniform attention): {dq}"


@pytest.mark.parametrize("B,S,p,n_slab", Q.ATTN_RANDOM_CASES)
def test_attention_yardsticks(B, S, p, n_slab):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    _, _, plain, e32, e64 = Q.attn_random_case(B, S, p, n_slab)
    _yardsticks([(n, Q.attn_rows(n, plain[n], B), Q.attn_rows(n, e32[n], B), Q.attn_rows(n, e64[n], B)) for n in Q.ATTN_OUTPUTS],
                f"attention B {B} S {S} p {p} slabs {n_slab}")


# ------------------------------------------------------------------------------------------------
# the whole trunk
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,L,FF", [(1, 1, 1, 128), (3, 7, 2, 256), (2, 32, 4, 384)])
def test_trunk_reference_matches_torch_encoder(B, S, L, FF):
    """nn.Embedding + nn.TransformerEncoder + mean in float64 and its autograd: pooled, the gradient of emb, of the position table and of
    every layer parameter as the kernels' operands give them"""
    torch.manual_seed(10 * B + S + L)
    layer = torch.nn.TransformerEncoderLayer(Q.E, Q.NH, dim_feedforward=FF, dropout=0.0, batch_first=True)
    enc = torch.nn.TransformerEncoder(layer, num_layers=L, norm=None, enable_nested_tensor=False).double()
    table = torch.nn.Embedding(40, Q.E).double()
    with torch.no_grad():
        for q in enc.parameters():                     # independent layers, non-trivial biases and LayerNorm parameters
            q.copy_(torch.randn_like(q) * (0.1 if q.dim() == 1 else 0.08))
            if q.dim() == 1 and q.numel() == Q.E:
                q.add_(0.7)
    emb = torch.randn(B, S, Q.E, dtype=torch.float64, requires_grad=True)
    ids = Q.trunk_pos_ids(S)
    dpooled = torch.randn(B, Q.E, dtype=torch.float64)
    pooled = enc(emb + table(ids)[None]).mean(1)
    pooled.backward(dpooled)
    d = lambda t: t.detach()
    layers = [dict(Wqkv=d(m.self_attn.in_proj_weight), bqkv=d(m.self_attn.in_proj_bias), Wo=d(m.self_attn.out_proj.weight), bo=d(m.self_attn.out_proj.bias),
                   W1=d(m.linear1.weight), b1=d(m.linear1.bias), W2=d(m.linear2.weight), b2=d(m.linear2.bias), g1=d(m.norm1.weight), be1=d(m.norm1.bias),
                   g2=d(m.norm2.weight), be2=d(m.norm2.bias)) for m in enc.layers]
    got = Q.trunk(d(emb), d(table.weight), ids, layers, Q.trunk_keep(0.0, 0, 0, B, S, FF, L), dpooled)
    _close(got["pooled"], d(pooled), "pooled")
    _close(got["demb"], emb.grad, "demb")
    dpos = torch.zeros(40, Q.E, dtype=torch.float64).index_add_(0, ids, got["demb"].sum(0))
    _close(dpos, table.weight.grad, "dpos")
    x = got["x0"]
    for m, t in zip(enc.layers, got["layers"]):
        who = f"layer {len(t)}"
        _close(t["dqkv"].t() @ x, m.self_attn.in_proj_weight.grad, who + " dWqkv")
        _close(t["dqkv"].sum(0), m.self_attn.in_proj_bias.grad, who + " dbqkv")
        _close(t["d_o"].t() @ t["ctx"], m.self_attn.out_proj.weight.grad, who + " dWo")
        _close(t["d_o"].sum(0), m.self_attn.out_proj.bias.grad, who + " dbo")
        _close(t["dh"].t() @ t["y1"], m.linear1.weight.grad, who + " dW1")
        _close(t["dh"].sum(0), m.linear1.bias.grad, who + " db1")
        _close(t["df"].t() @ t["h"], m.linear2.weight.grad, who + " dW2")
        _close(t["df"].sum(0), m.linear2.bias.grad, who + " db2")
        for lnp, norm in ((t["lnp1"], m.norm1), (t["lnp2"], m.norm2)):
            _close(lnp.sum(0)[0], norm.weight.grad, who + " dgamma")
            _close(lnp.sum(0)[1], norm.bias.grad, who + " dbeta")
        x = t["y2"]


def test_trunk_masks_follow_the_launch_row():
    """sequences b0 .. of a launch draw the masks of their launch row: a slice of a larger launch's masks"""
    full = Q.trunk_keep(0.5, Q.TRUNK_SITE, Q.RNG_WORD, 5, 3, 128, 2)
    part = Q.trunk_keep(0.5, Q.TRUNK_SITE, Q.RNG_WORD, 2, 3, 128, 2, b0=3)
    assert torch.equal(full["pos"][9:], part["pos"]) and 0 < (full["pos"] == 0).double().mean() < 1
    for f, p in zip(full["layers"], part["layers"]):
        assert torch.equal(f["attn"][3:], p["attn"]) and torch.equal(f["ffn"][9:], p["ffn"]) and torch.equal(f["ln1"][9:], p["ln1"]) and torch.equal(f["ln2"][9:], p["ln2"])
    ka, kl = Q.attn_keep(0.5, Q.trunk_seeds(Q.TRUNK_SITE, 2)[1]["seed_attn"], Q.trunk_seeds(Q.TRUNK_SITE, 2)[1]["seed_ln1"], Q.RNG_WORD, 5, 3)
    assert torch.equal(ka, full["layers"][1]["attn"]) and torch.equal(kl, full["layers"][1]["ln1"])
    assert torch.equal(Q.ffn_keep(0.5, Q.trunk_seeds(Q.TRUNK_SITE, 2)[0]["seed_ffn"], Q.RNG_WORD, 15, 128), full["layers"][0]["ffn"])


@pytest.mark.parametrize("B,S,L,FF", Q.TRUNK_RANDOM_CASES)
def test_trunk_yardsticks(B, S, L, FF):
    """rows are sequences; a ReLU gate that differs between the bf16 and the float64 evaluation is part of the yardstick, so the condition is
    that the rounding points ALONE (float64 accumulation) stay inside the GPU file's margin for every committed case"""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    _, plain, e32, e64 = Q.trunk_random_case(B, S, L, FF)
    _yardsticks([(n, Q.trunk_rows(a, B), Q.trunk_rows(b, B), Q.trunk_rows(c, B))
                 for (n, a), (_, b), (_, c) in zip(Q.trunk_tensors(plain), Q.trunk_tensors(e32), Q.trunk_tensors(e64))], f"trunk B {B} S {S} L {L} FF {FF}", cap=0.2)
