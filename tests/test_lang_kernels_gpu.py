"""Kernel-level tests of csrc/lang_encoder.hip — the pieces of the frozen MiniLM sentence encoder around its dense layers: the embedding sum +
LayerNorm, the masked multi-head attention and the masked mean pool — each against a few lines of float64 torch, at the sizes where a wave's
column loop, a workgroup's token quartet or the attention's LDS layout change shape, and with the sentences the fixtures never hold: a single
token, a hole in the mask, a sentence that is all padding.  The pattern of a case and the tolerance rule are in tests/kcheck.py.

The host-side bounds of kernels.embed_ln_fwd (token ids against the vocabulary, S against the position table) are tested on CPU tensors: they
raise before anything is launched, and nothing here launches a call that would read out of bounds."""
import pytest
import torch
import torch.nn.functional as F

from tests import kcheck as K
from tests.kcheck import compare, compare_rows, out_flat, refused, rnd, same_bits

gpu = pytest.mark.gpu

# Margins of margin * max(e_ref, 2^-23), e_ref = the float32 CPU evaluation of the same formula against float64 (tests/kcheck.py).
#   FAST 16: kernels built on rsqrtf / expf and butterfly wave sums (the embedding LayerNorm, the attention): the class of
#            tests/test_reductions_gpu.py — each is worth a few float32 roundings in another tree than torch's CPU code, and nothing larger is.
#   SUM   4: plain float32 sums and one division (the masked mean): only the summation order differs from the CPU's.
# A kernel that cannot meet its margin is a finding and gets a row here with the measured float32-CPU and GPU errors and the cause.
#   kernel                        what     cpu-f32     gpu        cause
#   (none)
MARGIN = {"FAST": 16.0, "SUM": 4.0}

F32 = torch.float32
LN_EPS = 1e-12                   # BertEmbeddings' LayerNorm


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    K.report("tests/test_lang_kernels_gpu.py")


def _gen(*key):
    """a generator seeded from the case's own parameters (stable across processes: no str hash)"""
    seed = 0
    for k in key:
        for ch in (k if isinstance(k, str) else repr(k)):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _in(dev, t, dtype, lead=0):
    """an input tensor inside a sentinel allocation (NaN for floats): a stray read that is consumed surfaces in the output"""
    return out_flat(dev, t.numel(), dtype, init=t, lead=lead).t.reshape(t.shape)


# ------------------------------------------------------------------------------------------------
# embedding sum + LayerNorm (hulc_embed_ln_fwd)
# ------------------------------------------------------------------------------------------------
VOCAB = 50


def _embed_ref(ids, word, pos, type0, gamma, beta, S, dt):
    """BertEmbeddings: (word[id] + type0) + pos[t % S], then LayerNorm (biased variance)"""
    T, D = ids.numel(), word.shape[1]
    word, pos, type0, gamma, beta = (t.to(dt) for t in (word, pos, type0, gamma, beta))
    v = (word[ids] + type0) + pos[torch.arange(T) % S]
    return F.layer_norm(v, (D,), gamma, beta, LN_EPS)


def _embed_tables(g, D, rows_pos):
    return (rnd(_randn(g, VOCAB, D), F32), rnd(_randn(g, rows_pos, D), F32), rnd(_randn(g, D), F32), rnd(0.5 + torch.rand(D, generator=g, dtype=torch.float64), F32),
            rnd(_randn(g, D), F32))


# D: 1 = a row of one element (variance 0: the output is beta); 63 / 64 / 65 = one column short of, exactly, one past a wave's first pass;
#    384 = MiniLM; 1024 = all sixteen register slots of every lane
# T: 1 and 5 = a partial last workgroup of four tokens; 8 = two full ones.   S: 1, 3 (the position wraps inside a workgroup) and T (it never wraps)
@gpu
@pytest.mark.parametrize("D", (1, 63, 64, 65, 384, 1024))
@pytest.mark.parametrize("T", (1, 5, 8))
@pytest.mark.parametrize("Sk", (1, 3, "T"))
def test_embed_ln_fwd(dev, D, T, Sk):
    from hulc2_amd import kernels as kn

    S = T if Sk == "T" else Sk
    what = f"embed_ln D={D} T={T} S={S}"
    g = _gen("embed", D, T, S)
    # the position table has a row for every t, not only for t % S: the rows past S hold other values, so an index that forgets the wrap reads
    # a wrong row, not memory outside the table
    word64, pos64, type64, ga64, be64 = _embed_tables(g, D, max(T, S) + 1)
    ids64 = torch.randint(0, VOCAB, (T,), generator=g)
    ids64[0], ids64[T - 1] = (0, VOCAB - 1) if T > 1 else (VOCAB - 1, VOCAB - 1)         # both ends of the vocabulary
    if T > 2:
        ids64[1] = 0
    ids = _in(dev, ids64, torch.int64)
    word, pos, type0, ga, be = (_in(dev, t, F32) for t in (word64, pos64, type64, ga64, be64))
    r64 = _embed_ref(ids64, word64, pos64, type64, ga64, be64, S, torch.float64)
    r32 = _embed_ref(ids64, word64, pos64, type64, ga64, be64, S, torch.float32)

    def call():
        out = out_flat(dev, T * D, F32)
        kn.embed_ln_fwd(ids, word, pos, type0, ga, be, LN_EPS, T, S, D, out.t.reshape(T, D))
        torch.cuda.synchronize()
        out.assert_guards(what)
        return out.value().reshape(T, D)

    y = call()
    if D == 1:
        assert torch.equal(y.cpu(), be64.float().expand(T, 1)), f"{what}: a one-element row normalises to beta exactly"
    compare("embed_ln_fwd", f"D={D}", y, r64, r32, MARGIN["FAST"])
    same_bits(y, call(), what)


@gpu
def test_embed_ln_fwd_refusals(dev):
    from hulc2_amd import kernels as kn

    g = _gen("embed refusals")
    message = "hulc_embed_ln_fwd: needs T, S > 0 and 0 < D <= 1024"
    for D, S in ((1025, 2), (64, 0)):
        T = 4
        word64, pos64, type64, ga64, be64 = _embed_tables(g, D, T)
        ids = _in(dev, torch.randint(0, VOCAB, (T,), generator=g), torch.int64)
        word, pos, type0, ga, be = (_in(dev, t, F32) for t in (word64, pos64, type64, ga64, be64))
        out = out_flat(dev, T * D, F32)
        refused(lambda: kn.embed_ln_fwd(ids, word, pos, type0, ga, be, LN_EPS, T, S, D, out.t.reshape(T, D)), message, out)


def test_embed_ln_fwd_host_bounds():
    """what the kernel indexes without looking — word[id], pos[t % S], row t of out — is bounded by the wrapper, on the host, before any launch
    (CPU tensors: a call that passed these checks would stop at the wrapper's device check, so nothing can be launched from here)"""
    from hulc2_amd import kernels as kn
    from hulc2_amd.lib import HulcKernelError

    T, S, D = 6, 3, 16
    g = _gen("embed host")
    word, pos, type0, ga, be = (t.float() for t in _embed_tables(g, D, S))
    good = torch.randint(0, VOCAB, (T,), generator=g)
    out = torch.full((T, D), 7.0)

    def attempt(exc, text, ids=good, word=word, pos=pos, S=S, T=T, out=out):
        with pytest.raises(exc) as ei:
            kn.embed_ln_fwd(ids, word, pos, type0, ga, be, LN_EPS, T, S, D, out)
        assert text in str(ei.value), f"expected {text!r}, got {ei.value}"

    bad = good.clone(); bad[2] = VOCAB
    attempt(ValueError, f"the vocabulary has {VOCAB} rows", ids=bad)
    bad = good.clone(); bad[T - 1] = -1
    attempt(ValueError, f"the vocabulary has {VOCAB} rows", ids=bad)
    attempt(ValueError, f"exceeds the position table's {S} rows", S=S + 1)
    attempt(ValueError, "token ids for T", T=T + 1, out=torch.zeros(T + 1, D))
    attempt(TypeError, "word is a contiguous fp32", word=word[:, :D - 1].contiguous())
    attempt(TypeError, "pos is a contiguous fp32", pos=pos.double())
    attempt(TypeError, "out is a contiguous fp32", out=torch.zeros(T - 1, D))
    attempt(TypeError, "contiguous int64", ids=good.int())
    attempt(HulcKernelError, "device memory only")          # in bounds: the next stop is the device check, still before the library
    assert torch.equal(out, torch.full((T, D), 7.0))


# ------------------------------------------------------------------------------------------------
# masked multi-head attention (hulc_mha_masked_fwd)
# ------------------------------------------------------------------------------------------------
def _mha_ref(qkv, mask, B, S, nhead, hd, dt):
    """softmax(q . k / sqrt(hd) + (mask ? 0 : finfo(float32).min)) v per sentence and head, BertSelfAttention's arithmetic (a sentence that is
    all padding gets the same addend on every key: the plain mean of V)"""
    D = nhead * hd
    q, k, v = (t.reshape(B, S, nhead, hd).permute(0, 2, 1, 3) for t in qkv.to(dt).reshape(B, S, 3, D).unbind(2))
    add = torch.where(mask.bool(), 0.0, torch.finfo(torch.float32).min).to(dt)
    p = torch.softmax(q @ k.transpose(-1, -2) / torch.tensor(hd, dtype=dt).sqrt() + add[:, None, None, :], dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * S, D)


def _masks(S):
    """three sentences: right padding down to a single token; a hole in the middle (the mask is not a prefix); all padding"""
    m = torch.zeros(3, S, dtype=torch.int32)
    m[0, 0] = 1
    m[1] = 1
    if S > 2:
        m[1, S // 3:max(S // 3 + 1, 2 * S // 3)] = 0
    return m


# S, hd, heads, score spread: 1 = unit scores; 30 = |q . k| / sqrt(hd) reaches 80 and beyond (exp overflows float32 without the running maximum)
MHA = [
    (1, 32, 12, 1.0),          # a single token: one key, softmax = 1
    (37, 32, 12, 1.0),         # MiniLM's heads on an odd length
    (37, 32, 12, 30.0),
    (128, 32, 2, 1.0),         # the longest sentence: every thread of the workgroup a query
    (5, 1, 3, 1.0),            # head dim 1: K and V rows of two floats in LDS
    (20, 64, 2, 30.0),         # the widest head
    (128, 64, 1, 1.0),         # 67,072 bytes of LDS: above the default dynamic limit, the launcher raises it
]


@gpu
@pytest.mark.parametrize("S,hd,nhead,spread", MHA)
def test_mha_masked_fwd(dev, S, hd, nhead, spread):
    from hulc2_amd import kernels as kn

    B, D = 3, nhead * hd
    what = f"mha S={S} hd={hd} heads={nhead} spread={spread}"
    g = _gen("mha", S, hd, nhead, spread)
    qkv64 = _randn(g, B * S, 3 * D)
    qkv64[:, :2 * D] *= spread ** 0.5
    qkv64 = rnd(qkv64, F32)
    m = _masks(S)
    r64, r32 = _mha_ref(qkv64, m, B, S, nhead, hd, torch.float64), _mha_ref(qkv64, m, B, S, nhead, hd, torch.float32)
    if spread > 1:
        top = (qkv64[:, :D].reshape(B, S, nhead, hd).permute(0, 2, 1, 3) @ qkv64[:, D:2 * D].reshape(B, S, nhead, hd).permute(0, 2, 3, 1)).abs().max().item() / hd ** 0.5
        assert top > 80.0, f"the largest score is {top:.1f}: the case is meant to need the maximum subtraction"
    v = qkv64[:, 2 * D:].reshape(B, S, D)
    assert torch.allclose(r64.reshape(B, S, D)[2], v[2].mean(0, keepdim=True).expand(S, D), rtol=0, atol=1e-12), "all padding: the plain mean of V"
    qkv, mask = _in(dev, qkv64, F32), _in(dev, m, torch.int32)

    def call():
        out = out_flat(dev, B * S * D, F32)
        kn.mha_masked_fwd(qkv, mask, B, S, nhead, hd, out.t.reshape(B * S, D))
        torch.cuda.synchronize()
        out.assert_guards(what)
        return out.value().reshape(B * S, D)

    y = call()
    compare_rows("mha_masked_fwd", f"S={S} hd={hd}", y, r64, r32, MARGIN["FAST"])
    same_bits(y, call(), what)


@gpu
def test_mha_masked_fwd_refusals(dev):
    from hulc2_amd import kernels as kn

    g = _gen("mha refusals")
    message = "hulc_mha_masked_fwd: needs S <= 128 and head dim <= 64"
    for S, hd, nhead in ((129, 32, 1), (4, 65, 1), (4, 32, 0)):
        D = max(nhead, 1) * hd
        qkv, mask = _in(dev, _randn(g, S, 3 * D), F32), _in(dev, torch.ones(1, S, dtype=torch.int32), torch.int32)
        out = out_flat(dev, S * D, F32)
        refused(lambda: kn.mha_masked_fwd(qkv, mask, 1, S, nhead, hd, out.t.reshape(S, D)), message, out)


# ------------------------------------------------------------------------------------------------
# masked mean pool (hulc_masked_mean_fwd)
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("D", (1, 127, 128, 129, 384))
@pytest.mark.parametrize("S", (1, 37))
def test_masked_mean_fwd(dev, D, S):
    from hulc2_amd import kernels as kn

    B = 4
    what = f"masked_mean D={D} S={S}"
    g = _gen("mean", D, S)
    m = torch.cat([torch.ones(1, S, dtype=torch.int32), _masks(S)])           # a full sentence, a single token, a hole, all padding
    x64 = rnd(_randn(g, B, S, D) + 0.5, F32)
    live = m.bool()[:, :, None].expand(B, S, D)
    ref = lambda dt: torch.where(live, x64.to(dt), torch.zeros((), dtype=dt)).sum(1) / m.sum(1, keepdim=True).to(dt).clamp_min(1e-9)
    x = _in(dev, torch.where(live, x64, torch.full((), float("nan"), dtype=torch.float64)), F32)      # padded tokens hold NaN: reading one shows
    mask = _in(dev, m, torch.int32)

    def call():
        out = out_flat(dev, B * D, F32)
        kn.masked_mean_fwd(x, mask, B, S, D, out.t.reshape(B, D))
        torch.cuda.synchronize()
        out.assert_guards(what)
        return out.value().reshape(B, D)

    y = call()
    assert not y[3].any(), f"{what}: a sentence that is all padding pools to exactly zero"
    compare("masked_mean_fwd", f"D={D} S={S}", y, ref(torch.float64), ref(torch.float32), MARGIN["SUM"])
    same_bits(y, call(), what)


@gpu
def test_masked_mean_fwd_refusals(dev):
    from hulc2_amd import kernels as kn

    x, mask = _in(dev, torch.ones(2, 3, 8, dtype=torch.float64), F32), _in(dev, torch.ones(2, 3, dtype=torch.int32), torch.int32)
    out = out_flat(dev, 16, F32)
    for B, S, D in ((0, 3, 8), (2, 0, 8), (2, 3, 0)):
        refused(lambda: kn.masked_mean_fwd(x, mask, B, S, D, out.t.reshape(2, 8)), "hulc_masked_mean_fwd: bad shape", out)
