"""CPU references of the fused sequence kernels (csrc/ffn_fused.hip, csrc/txl_fused.hip + csrc/txl_attn.h, csrc/txl_block.hip,
csrc/rnn_wavefront.hip), used by tests/test_ffn_kernel_gpu.py, tests/test_txl_attn_kernel_gpu.py, tests/test_txl_block_kernel_gpu.py and
tests/test_rnn_kernel_gpu.py and checked against torch's own float64 modules by tests/test_seqref_cpu.py.

Three things per kernel:
  * a PLAIN float64 reference of the operation on operands rounded to their storage type (the rnd() convention of tests/kcheck.py): what
    the random GPU cases are compared with;
  * a ROUNDING-POINT EMULATION: the same formulas with the kernel's documented bf16 rounding points inserted and the accumulation type
    (float32 or float64) as a parameter.  With float32 accumulation its error against the plain reference is the yardstick `e_ref` of
    kcheck.compare_rows; it is never an expected value of a random case;
  * LATTICE BUILDERS: integer-valued operands for which the builder asserts in float64 that every accumulation satisfies
    sum |terms| < 2^24.  Then fp32 arithmetic in any order is exact, each bf16 rounding point rounds an exactly known value (round to nearest
    even, which .to(torch.bfloat16) reproduces), and the float64 emulation is what the kernel must give BIT FOR BIT.

Dropout masks come from oracle/counter_rng.py with the index formulas of the kernels' headers (feed-forward: token * FF + hidden unit;
attention probabilities: ((b H + h) S + i) S + j; residual branches and the position add: token * E + feature).
"""
import numpy as np
import torch

from oracle import counter_rng as R

EXACT = float(2 ** 24)


def bf(t: torch.Tensor) -> torch.Tensor:
    """round to bf16 (nearest even), keep the dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def _ident(t):
    return t


def _gran(t: torch.Tensor) -> float:
    """the largest power of two of which every element of t is a multiple (inf for an all-zero tensor)"""
    nz = t.double()[t != 0]
    if nz.numel() == 0:
        return float("inf")
    m, e = torch.frexp(nz)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()
    return 2.0 ** float((torch.log2(low) + e - 53).min())


def _assert_exact(what: str, a: torch.Tensor, b: torch.Tensor, extra=None) -> float:
    """the lattice condition of a (batched) product a @ b (+ extra): with u = the product of the operands' lattice units (the largest powers
    of two dividing all their elements; also dividing `extra`), every term and partial sum is a multiple of u, and
    sum over k of |a[m, k] b[k, n]| (+ |extra|) < 2^24 u for every output element, evaluated in float64 - so fp32 holds every partial sum
    exactly in any order.  Returns the largest sum in units of u."""
    s = a.double().abs() @ b.double().abs()
    u = _gran(a) * _gran(b)
    if extra is not None:
        s = s + extra.double().abs()
        u = min(u, _gran(extra))
    if s.numel() == 0 or not s.any():
        return 0.0
    m = float(s.max()) / u
    assert m < EXACT, f"lattice {what}: sum |terms| reaches {m:.0f} units >= 2^24, fp32 accumulation is no longer exact"
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# feed-forward block   f = dropout(relu(x W1^T + b1)) W2^T + b2   and every output of hulc_ffn_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def ffn_keep(p: float, seed: int, word: int, T: int, FF: int) -> torch.Tensor:
    """keep-scales (T, FF) float64 of the hidden activation: counter RNG on (seed ^ word, token * FF + unit); all ones for p = 0"""
    if p <= 0.0:
        return torch.ones(T, FF, dtype=torch.float64)
    idx = np.arange(T * FF, dtype=np.uint64).reshape(T, FF)
    return torch.from_numpy(R.dropout_scale(int(seed) ^ (int(word) & R.MASK64), idx, p).astype(np.float64))


def ffn(x, W1, b1, W2, b2, df, keep, acc=torch.float64, emulate=False, check=None):
    """x, df (T, 128), W1 (FF, 128), b1 (FF), W2 (128, FF), b2 (128), keep (T, FF): float64 tensors holding storage-rounded values.
    emulate: the kernel's bf16 rounding points (x, df -> bf16; h, dh -> bf16 after gate and dropout; db1 from the unrounded dh) and
    products accumulated in `acc`.  check(name, a, b, extra): called for every product (the lattice builders' 2^24 assertion).
    -> dict of float64 tensors: f, dx, dW1, db1, dW2, the hidden-slice partials f_slab / dx_slab (FF / 128, T, 128) (b2 in slice 0 of
    f_slab) and the intermediates z, h, dh."""
    r = bf if emulate else _ident
    c = lambda t: t.to(acc)
    check = check or (lambda *a: None)
    T, FF = x.shape[0], W1.shape[0]
    xr, dfr, W1a, W2a, kp = r(c(x)), r(c(df)), c(W1), c(W2), c(keep)
    check("z", xr, W1a.t(), c(b1))
    z = xr @ W1a.t() + c(b1)
    gate = (z > 0).to(acc)
    h_full = z * gate * kp
    h = r(h_full)
    check("dhd", dfr, W2a)
    dh_full = (dfr @ W2a) * gate * kp
    dh = r(dh_full)
    ns = FF // 128
    f_slab = torch.stack([h[:, s * 128:(s + 1) * 128] @ W2a[:, s * 128:(s + 1) * 128].t() for s in range(ns)])
    f_slab[0] += c(b2)
    dx_slab = torch.stack([dh[:, s * 128:(s + 1) * 128] @ W1a[s * 128:(s + 1) * 128] for s in range(ns)])
    check("f", h, W2a.t(), c(b2))
    check("dx", dh, W1a)
    check("dW1", dh.t(), xr)
    check("dW2", dfr.t(), h)
    check("db1", dh_full.t(), torch.ones(T, 1, dtype=acc))
    out = dict(z=z, h=h, dh=dh, f_slab=f_slab, dx_slab=dx_slab, f=f_slab.sum(0), dx=dx_slab.sum(0),
               dW1=dh.t() @ xr, db1=dh_full.sum(0), dW2=dfr.t() @ h)
    return {k: v.double() for k, v in out.items()}


def ffn_lattice(T: int, FF: int, seed: int, p: float = 0.0, rng_seed: int = 0, word: int = 0, big: bool = False):
    """integer operands: x in [-4, 4], W1 in [-2, 2], W2 in [-1, 1], b1 in [-8, 8], b2 in [-3, 3], df in [-3, 3] (big: x in [-7, 7] and
    W1 in [-3, 3], hidden values well above 256 so that their bf16 rounding, exact ties included, is exercised).  p is 0 or 0.5 (scale
    exactly 2).  Asserts the 2^24 condition for every product and that float32 and float64 emulations agree bit for bit.
    -> (operands dict, expected dict = the float64 emulation, stats dict)"""
    assert p in (0.0, 0.5)
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    xa, wa = (7, 3) if big else (4, 2)
    ops = dict(x=ri(-xa, xa, T, 128), W1=ri(-wa, wa, FF, 128), b1=ri(-8, 8, FF), W2=ri(-1, 1, 128, FF), b2=ri(-3, 3, 128), df=ri(-3, 3, T, 128))
    keep = ffn_keep(p, rng_seed, word, T, FF)
    sums = {}

    def check(name, a, b, extra=None):
        sums[name] = _assert_exact(f"ffn {name} (T {T}, FF {FF})", a, b, extra)

    want = ffn(**ops, keep=keep, acc=torch.float64, emulate=True, check=check)
    w32 = ffn(**ops, keep=keep, acc=torch.float32, emulate=True)
    for k in want:
        assert torch.equal(want[k], w32[k]), f"ffn lattice (T {T}, FF {FF}): float32 and float64 emulations differ in {k}"
    plain = ffn(**ops, keep=keep)
    hf = plain["h"]                                                  # the unrounded hidden values
    odd = (hf >= 256) & (hf < 512) & (hf % 2 == 1)
    stats = dict(sums=sums, h_max=float(hf.max()), ties=int(odd.sum()), f_max=float(want["f"].abs().max()),
                 rounded=int((bf(hf) != hf).sum()))
    ops["keep"] = keep
    return ops, want, stats


def ffn_random(T: int, FF: int, seed: int, p: float = 0.0, rng_seed: int = 0, word: int = 0):
    """the random case at the model's magnitudes.  x, W1, b1 sit on a dyadic grid (x: multiples of 2^-4 in [-2, 2]; W1: multiples of 2^-6
    in [-1/8, 1/8]; b1: multiples of 2^-10 in [-1/8, 1/8]) so that the pre-activation is exact in fp32 and no ReLU gate can flip between
    the kernel and the reference (asserted); W2, b2, df are continuous.  -> (operands rounded to storage, plain, emu32, emu64)"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    ops = dict(x=torch.round(u(T, 128) * 32) / 16, W1=torch.round(u(FF, 128) * 8) / 64, b1=torch.round(u(FF) * 128) / 1024,
               W2=(u(128, FF) * FF ** -0.5).to(torch.bfloat16).double(), b2=(u(128) * 0.1).float().double(), df=u(T, 128).float().double())
    assert torch.equal(ops["x"], bf(ops["x"])) and torch.equal(ops["W1"], bf(ops["W1"]))
    keep = ffn_keep(p, rng_seed, word, T, FF)
    plain = ffn(**ops, keep=keep)
    e32 = ffn(**ops, keep=keep, acc=torch.float32, emulate=True)
    e64 = ffn(**ops, keep=keep, acc=torch.float64, emulate=True)
    assert torch.equal(plain["z"], e32["z"]), "the dyadic pre-activation is not exact in fp32: a gate could flip"
    ops["keep"] = keep
    return ops, plain, e32, e64


# ---------------------------------------------------------------------------------------------------------------------------------
# wavefront recurrence, as include/hulc2_amd.h states it
# ---------------------------------------------------------------------------------------------------------------------------------
def rnn_sweep(S, B, H, wA, wB1, wB2, add1=None, add1c=None, bias1=(None, None), bias2=(None, None), mask1=None, mask2=None, relu=False,
              acc=torch.float64, emulate=False, check=None):
    """State rows z[0 .. S+1] (S + 2, B, 2H) in SWEEP order (row r is wave step r's input whichever way the buffer is walked).
    wA, wB1, wB2 (H, H): element (n, k) multiplies input k of output n (the caller undoes a transposed storage).  add1, mask1, mask2
    are indexed by wave step: (S, B, H), (S, B, H) and (S + 1, B, H) (mask2[0] is never used).  Row 0 is zero; wave step tau writes
          first half  (tau < S):  f1(z_tau[:, :H] wA^T + add1[tau] + bias1a + bias1b + add1c)
          second half (tau >= 1): f2(z_tau[:, :H] wB1^T + z_tau[:, H:] wB2^T + bias2a + bias2b),   zero at tau = 0
    of row tau + 1; f keeps where mask[tau] > 0 when a mask is given, else ReLU when relu.  The first half of row S+1 is never produced
    and stays zero (what zero_edges leaves there).  emulate: the state is rounded to bf16 once per wave step, as the operand of the next
    step's products (the stored fp32 row is not rounded); products accumulate in `acc`."""
    c = lambda t: None if t is None else t.to(acc)
    check = check or (lambda *a: None)
    wA, wB1, wB2, add1, add1c, mask1, mask2 = map(c, (wA, wB1, wB2, add1, add1c, mask1, mask2))
    zero = torch.zeros(H, dtype=acc)
    b1 = sum((c(b) for b in bias1 if b is not None), zero)
    b2 = sum((c(b) for b in bias2 if b is not None), zero)
    if add1c is not None:
        b1 = b1 + add1c                                               # (B, H)
    z = torch.zeros(S + 2, B, 2 * H, dtype=acc)
    for tau in range(S + 1):
        zin = bf(z[tau]) if emulate else z[tau]
        if tau < S:
            e = b1 + (add1[tau] if add1 is not None else 0)
            check(f"first[{tau}]", zin[:, :H], wA.t(), e.expand(B, H))
            v = zin[:, :H] @ wA.t() + e
            v = torch.where(mask1[tau] > 0, v, torch.zeros_like(v)) if mask1 is not None else (v.clamp_min(0) if relu else v)
            z[tau + 1, :, :H] = v
        if tau >= 1:
            check(f"second[{tau}]", zin, torch.cat([wB1, wB2], 1).t(), b2.expand(B, H))
            v = zin[:, :H] @ wB1.t() + zin[:, H:] @ wB2.t() + b2
            v = torch.where(mask2[tau] > 0, v, torch.zeros_like(v)) if mask2 is not None else (v.clamp_min(0) if relu else v)
            z[tau + 1, :, H:] = v
    return z.double()


def sparse_sign_matrix(H: int, g: torch.Generator, nnz: int) -> torch.Tensor:
    """(H, H) float64 with `nnz` or `nnz + 1` random +-1 entries per row (repeated columns merge: an entry may be 0 or +-2)"""
    w = torch.zeros(H, H, dtype=torch.float64)
    for j in range(nnz + 1):
        cols = torch.randint(0, H, (H,), generator=g)
        sign = torch.randint(0, 2, (H,), generator=g).double() * 2 - 1
        if j == nnz:
            sign = sign * torch.randint(0, 2, (H,), generator=g).double()
        w[torch.arange(H), cols] += sign
    return w


def rnn_lattice(S: int, B: int, seed: int, backward: bool, H: int = 2048, nnz: int = 3, amp: int = 3):
    """integer operands of one sweep.  Forward mode: relu, integer add1 in [-amp, amp], add1c in [-2, 2], four small negative biases.
    Backward mode: masks in {-1, 0, 0.5, 3} (kept where > 0), integer add1, no biases.  Weights have nnz .. nnz + 1 random +-1 per row.
    Asserts the 2^24 condition at every wave step and that the float32 and float64 emulations agree bit for bit.
    -> (operands dict for rnn_sweep, expected rows (S + 2, B, 2H) float64, stats dict)"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    ops = dict(wA=sparse_sign_matrix(H, g, nnz), wB1=sparse_sign_matrix(H, g, nnz), wB2=sparse_sign_matrix(H, g, nnz), add1=ri(-amp, amp, S, B, H))
    if backward:
        vals = torch.tensor([-1.0, 0.0, 0.5, 3.0], dtype=torch.float64)
        ops.update(mask1=vals[torch.randint(0, 4, (S, B, H), generator=g)], mask2=vals[torch.randint(0, 4, (S + 1, B, H), generator=g)], relu=False)
    else:
        ops.update(add1c=ri(-2, 2, B, H), bias1=(ri(-1, 0, H), ri(-1, 0, H)), bias2=(ri(-1, 0, H), ri(-1, 0, H)), relu=True)
    sums = []

    def check(name, a, b, extra=None):
        sums.append(_assert_exact(f"rnn {name} (S {S}, B {B})", a, b, extra))

    want = rnn_sweep(S, B, H, **ops, acc=torch.float64, emulate=True, check=check)
    w32 = rnn_sweep(S, B, H, **ops, acc=torch.float32, emulate=True)
    assert torch.equal(want, w32), f"rnn lattice (S {S}, B {B}): float32 and float64 emulations differ"
    a = want.abs()
    stats = dict(sum_max=max(sums), z_max=float(a.max()), nonzero=float((want[1:S + 1] != 0).double().mean()),
                 ties=int(((a >= 256) & (a < 512) & (a % 2 == 1)).sum()), rounded=int((bf(want) != want).sum()))
    return ops, want, stats


def rnn_random(S: int, B: int, seed: int, backward: bool, H: int = 2048):
    """the random case at the model's magnitudes: weights U(-1, 1) / sqrt(H) rounded to bf16, add1 ~ N(0, 1) fp32, biases U(-1, 1) / sqrt(H).
    Forward mode uses relu (the case is forward-only: its gates are the kernel's own); backward mode takes its gates as masks, drawn
    from N(0, 1) (kept where > 0), so no gate depends on computed values.  -> (operands, plain float64 rows, emu32 rows, emu64 rows)"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()
    k = H ** -0.5
    w = lambda: (u(H, H) * k).to(torch.bfloat16).double()
    ops = dict(wA=w(), wB1=w(), wB2=w(), add1=n(S, B, H))
    if backward:
        ops.update(mask1=n(S, B, H), mask2=n(S + 1, B, H), relu=False)
    else:
        b = lambda: (u(H) * k).float().double()
        ops.update(add1c=n(B, H), bias1=(b(), b()), bias2=(b(), b()), relu=True)
    plain = rnn_sweep(S, B, H, **ops)
    e32 = rnn_sweep(S, B, H, **ops, acc=torch.float32, emulate=True)
    e64 = rnn_sweep(S, B, H, **ops, acc=torch.float64, emulate=True)
    return ops, plain, e32, e64


def rnn_rows(z: torch.Tensor, S: int) -> torch.Tensor:
    """the rows of kcheck.compare_rows for a state buffer in sweep order: (wave step, batch row, half) of everything the sweep produces
    (rows 1 .. S+1 without the first half of row S+1 and the structurally zero second half of row 1) -> (n, H)"""
    Sp2, B, H2 = z.shape
    H = H2 // 2
    first = z[1:S + 1, :, :H].reshape(-1, H)
    second = z[2:S + 2, :, H:].reshape(-1, H)
    return torch.cat([first, second], 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# attention half of the post-norm layer   y = LayerNorm(x + dropout(out_proj(MHA(x))))   (csrc/txl_attn.h), d_model 128, 8 heads of 16
# ---------------------------------------------------------------------------------------------------------------------------------
E, NH, HD = 128, 8, 16


def attn_keep(p: float, seed_attn: int, seed_ln: int, word: int, B: int, S: int, b0: int = 0):
    """keep-scales of the attention probabilities (B, NH, S, S), index ((b NH + h) S + i) S + j, and of the out_proj residual branch (B S, E),
    index token * E + feature, for sequences b0 .. b0 + B - 1 of a launch; ones for p = 0"""
    if p <= 0.0:
        return torch.ones(B, NH, S, S, dtype=torch.float64), torch.ones(B * S, E, dtype=torch.float64)
    w = int(word) & R.MASK64
    ia = np.arange(b0 * NH * S * S, (b0 + B) * NH * S * S, dtype=np.uint64).reshape(B, NH, S, S)
    il = np.arange(b0 * S * E, (b0 + B) * S * E, dtype=np.uint64).reshape(B * S, E)
    return (torch.from_numpy(R.dropout_scale(int(seed_attn) ^ w, ia, p).astype(np.float64)),
            torch.from_numpy(R.dropout_scale(int(seed_ln) ^ w, il, p).astype(np.float64)))


def _heads(t, B, S):
    return t.reshape(B, S, NH, HD).permute(0, 2, 1, 3)                # (B, NH, S, HD)


def _tokens(t, B, S):
    return t.permute(0, 2, 1, 3).reshape(B * S, E)


def _qkvp(xr, Wqkv, bqkv, B, S, r, p_floor=0.0):
    """the projections as the kernel holds them (q scaled by 1/4; all three rounded at `r`) and the softmax P (B, NH, S query, S key)"""
    qkv = xr @ Wqkv.t() + bqkv
    q, k, v = r((qkv[:, :E]) * 0.25), r(qkv[:, E:2 * E]), r(qkv[:, 2 * E:])
    qh, kh, vh = _heads(q, B, S), _heads(k, B, S), _heads(v, B, S)
    s = qh @ kh.transpose(-1, -2)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    P = e * (1.0 / e.sum(-1, keepdim=True))
    if p_floor:                                                       # what underflows in the kernel's fp32 exp (the permutation lattice)
        P = torch.where(P < p_floor, torch.zeros_like(P), P)
    return qh, kh, vh, P


def attn_fwd(x, Wqkv, bqkv, Wo, bo, gamma, beta, eps, B, S, keep_attn, keep_ln, acc=torch.float64, emulate=False, check=None, p_floor=0.0):
    """x (B S, E) rows b S + s; Wqkv (3E, E), Wo (E, E): float64 tensors of storage-rounded values.  emulate: the kernel's bf16 rounding
    points (x as the projections' operand, q / 4, k, v, P after dropout, ctx) and `acc` arithmetic; the residual adds the UNROUNDED x.
    -> dict y, pre (B S, E), mean, rstd (B S), ctx (B S, E) (bf16 values when emulating: what the kernel stores), float64"""
    r = bf if emulate else _ident
    c = lambda t: t.to(acc)
    check = check or (lambda *a: None)
    x, Wqkv, bqkv, Wo, bo, gamma, beta, ka, kl = map(c, (x, Wqkv, bqkv, Wo, bo, gamma, beta, keep_attn, keep_ln))
    check("qkv", r(x), Wqkv.t(), bqkv.expand(B * S, 3 * E))
    qh, kh, vh, P = _qkvp(r(x), Wqkv, bqkv, B, S, r, p_floor)
    Pd = r(P * ka)
    check("ctx", Pd, vh)
    ctx = r(_tokens(Pd @ vh, B, S))
    check("o", ctx, Wo.t(), bo.expand(B * S, E))
    pre = x + (ctx @ Wo.t() + bo) * kl
    mean = pre.mean(-1)
    rstd = torch.rsqrt(((pre - mean[:, None]) ** 2).mean(-1) + eps)
    y = (pre - mean[:, None]) * rstd[:, None] * gamma + beta
    return {k: v.double() for k, v in dict(y=y, pre=pre, mean=mean, rstd=rstd, ctx=ctx, P=P).items()}


def ln_bwd(dy, pre, mean, rstd, gamma, B):
    """LayerNorm backward from the saved statistics -> dpre (T, E), per-sequence partials (B, 2, E) = {sum dy xhat, sum dy}"""
    xh = (pre - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    s1, s2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    dpre = rstd[:, None] * (g - s1 - xh * s2)
    part = torch.stack([(dy * xh).reshape(B, -1, E).sum(1), dy.reshape(B, -1, E).sum(1)], 1)
    return dpre, part


def attn_bwd(x, Wqkv, bqkv, Wo, gamma, B, S, keep_attn, keep_ln, pre, mean, rstd, dy, slabs=None, acc=torch.float64, emulate=False, check=None, p_floor=0.0):
    """backward of attn_fwd from the kept pre / mean / rstd (inputs of the launcher: a test may choose them) and dy (+ the partial slabs
    (n, B S, E), summed onto it).  emulate: bf16 at d_o, dctx, dS, P after dropout, dq, dk, dv and the recomputed q / 4, k, v; `acc` arithmetic.
    -> dict dx (B S, E), d_o (B S, E), dqkv (B S, 3E), ln_partial (B, 2, E), float64"""
    r = bf if emulate else _ident
    c = lambda t: t.to(acc)
    check = check or (lambda *a: None)
    x, Wqkv, bqkv, Wo, gamma, ka, kl, pre, mean, rstd, dy = map(c, (x, Wqkv, bqkv, Wo, gamma, keep_attn, keep_ln, pre, mean, rstd, dy))
    if slabs is not None and slabs.shape[0]:
        check("dy + slabs", torch.ones(1, slabs.shape[0] + 1, dtype=acc), torch.cat([dy[None], c(slabs)], 0).reshape(slabs.shape[0] + 1, -1))
        dy = dy + c(slabs).sum(0)
    dpre, part = ln_bwd(dy, pre, mean, rstd, gamma, B)
    d_o = r(dpre * kl)
    check("dctx", d_o, Wo)
    dctx = r(d_o @ Wo)
    qh, kh, vh, P = _qkvp(r(x), Wqkv, bqkv, B, S, r, p_floor)
    dch = _heads(dctx, B, S)
    check("dP", dch, vh.transpose(-1, -2))
    dP = dch @ vh.transpose(-1, -2)                                  # (B, NH, S query, S key)
    check("rs", dP * ka * P, torch.ones(S, 1, dtype=acc))
    rs = (dP * ka * P).sum(-1, keepdim=True)
    dS = r(P * (dP * ka - rs))
    Pd = r(P * ka)
    check("dv", Pd.transpose(-1, -2), dch)
    check("dq", dS, kh)
    check("dk", dS.transpose(-1, -2), qh)
    dv = r(Pd.transpose(-1, -2) @ dch)
    dq = r((dS @ kh) * 0.25)
    dk = r(dS.transpose(-1, -2) @ qh)
    dqkv = torch.cat([_tokens(dq, B, S), _tokens(dk, B, S), _tokens(dv, B, S)], 1)
    check("dx", dqkv, Wqkv, dpre)
    dx = dpre + dqkv @ Wqkv
    return {k: v.double() for k, v in dict(dx=dx, d_o=d_o, dqkv=dqkv, ln_partial=part, dy_total=dy).items()}


def hadamard_codes() -> torch.Tensor:
    """32 code vectors of +-1 and width 16 with pairwise dot products <= 0: the rows of the 16 x 16 Hadamard matrix and their negations"""
    h = torch.ones(1, 1, dtype=torch.float64)
    for _ in range(4):
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    c = torch.cat([h, -h], 0)
    d = c @ c.t()
    assert (d.diagonal() == 16).all() and (d - 16 * torch.eye(32, dtype=torch.float64)).max() <= 0
    return c


def perm_targets(S: int) -> torch.Tensor:
    """(NH, S): head h's query i attends to key (i + shift_h) mod S, a non-identity, non-involutive permutation (S >= 3)"""
    shifts = [k for k in range(1, S) if (2 * k) % S != 0]
    assert shifts, "a non-involutive cyclic shift needs S >= 3"
    return torch.stack([(torch.arange(S) + shifts[h % len(shifts)]) % S for h in range(NH)])


ATTN_KINDS = ("single", "uniform", "perm")


def attn_lattice(B: int, S: int, kind: str, seed: int, p: float = 0.0, seeds=(0, 0), word: int = 0, n_slab: int = 0, backward: bool = True):
    """structured cases in which softmax is exact, on integer x, Wv, bv, Wo, bo, gamma, beta:
      single   S = 1: the one probability is 1;
      uniform  Wq = 0, bq = 0, S a power of two: every score is 0, P = 1 / S exactly;
      perm     features 0 .. 31 of x are the one-hot position, Wq / Wk map it to +-1 codes of width 16 (code scale 32 in q): the target key
               (i + shift_h) mod S scores 0.25 * 32 * 16 = 128, every other key <= 0, so exp underflows to zero in fp32 (any denormal residue
               of a wider type vanishes in the bf16 rounding of P) and P is exactly one-hot.
    p is 0 or 0.5.  Forward: ctx and pre are exact (asserted: 2^24 condition, float32 emulation == float64 emulation); y / mean / rstd are
    the LayerNorm of an exactly known pre.  Backward from pre = 0, mean = 0, rstd = 1 and an integer dy (+ n_slab integer slabs) whose
    gamma-weighted rows sum to multiples of 128 (gamma is 1 on the last 32 features, which absorb the correction): LayerNorm backward is dy gamma - mean(dy gamma), and d_o, dqkv, dx, ln_partial are exact.
    backward = False: forward only (bops, bw = None): uniform attention over 32 keys leaves dS on a lattice of 2^-10 and below, too fine for
    the 2^24 condition of dq.
    -> (operands, forward expected, backward operands, backward expected, stats)"""
    assert p in (0.0, 0.5) and kind in ATTN_KINDS
    assert kind != "single" or S == 1
    assert kind != "uniform" or S & (S - 1) == 0
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    T = B * S
    x = ri(-4, 4, T, E)
    Wq, Wk, bq, bk = ri(-1, 1, E, E), ri(-1, 1, E, E), ri(-2, 2, E), ri(-2, 2, E)
    if kind == "uniform":
        Wq, bq = torch.zeros(E, E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    if kind == "perm":
        codes, tgt = hadamard_codes(), perm_targets(S)
        x[:, :32] = 0
        x[torch.arange(T), torch.arange(T) % S] = 1
        Wq, Wk, bq, bk = torch.zeros(E, E, dtype=torch.float64), torch.zeros(E, E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
        for h in range(NH):
            Wq[h * HD:(h + 1) * HD, :S] = 32 * codes[tgt[h]].t()
            Wk[h * HD:(h + 1) * HD, :S] = codes[:S].t()
    gamma = torch.tensor([1.0, -1.0, 2.0, -2.0], dtype=torch.float64)[torch.randint(0, 4, (E,), generator=g)]
    gamma[96:] = 1.0
    ops = dict(x=x, Wqkv=torch.cat([Wq, Wk, ri(-2, 2, E, E)], 0), bqkv=torch.cat([bq, bk, ri(-3, 3, E)]), Wo=ri(-1, 1, E, E), bo=ri(-3, 3, E),
               gamma=gamma, beta=ri(-2, 2, E), eps=1e-5, B=B, S=S)
    ka, kl = attn_keep(p, seeds[0], seeds[1], word, B, S)
    sums = {}

    def check(name, a, b, extra=None):
        sums[name] = _assert_exact(f"attention {kind} {name} (B {B}, S {S})", a, b, extra)

    floor = 2.0 ** -126                                               # exp(-128) is zero in fp32; float64 would keep 2.6e-56
    fw = attn_fwd(**ops, keep_attn=ka, keep_ln=kl, acc=torch.float64, emulate=True, check=check, p_floor=floor)
    fw32 = attn_fwd(**ops, keep_attn=ka, keep_ln=kl, acc=torch.float32, emulate=True)
    for k in ("ctx", "pre"):
        assert torch.equal(fw[k], fw32[k]), f"attention lattice {kind} (B {B}, S {S}): float32 and float64 emulations differ in {k}"
    Pd = bf(fw["P"] * ka)
    if kind == "perm":
        hot = torch.zeros(NH, S, S, dtype=torch.float64)
        hot[torch.arange(NH)[:, None], torch.arange(S)[None], tgt] = 1
        assert torch.equal(Pd, hot * ka), "the permutation case is not exactly one-hot"
    else:
        assert torch.equal(Pd, ka / S), "the probabilities are not exactly 1 / S"
    ops.update(keep_attn=ka, keep_ln=kl)
    if not backward:
        return ops, fw, None, None, dict(sums=sums, ctx_max=float(fw["ctx"].abs().max()), pre_max=float(fw["pre"].abs().max()))
    ops.pop("keep_attn"), ops.pop("keep_ln")
    # ---- backward operands
    total = ri(-2, 2, T, E)
    rest = (total[:, :96] * gamma[:96]).sum(-1)
    corr = ((-rest + 64) % 128) - 64                                 # in [-64, 63], spread over the 32 columns with gamma = 1: entries in [-2, 2]
    total[:, 96:] = torch.div(corr, 32, rounding_mode="floor")[:, None] + (torch.arange(32)[None] < (corr % 32)[:, None]).double()
    assert not ((total * gamma).sum(-1) % 128).any()
    slabs = ri(-3, 3, n_slab, T, E)
    bops = dict(pre=torch.zeros(T, E, dtype=torch.float64), mean=torch.zeros(T, dtype=torch.float64), rstd=torch.ones(T, dtype=torch.float64),
                dy=total - slabs.sum(0), slabs=slabs)
    common = dict(x=x, Wqkv=ops["Wqkv"], bqkv=ops["bqkv"], Wo=ops["Wo"], gamma=gamma, B=B, S=S, keep_attn=ka, keep_ln=kl)
    bw = attn_bwd(**common, **bops, acc=torch.float64, emulate=True, check=check, p_floor=floor)
    bw32 = attn_bwd(**common, **bops, acc=torch.float32, emulate=True)
    for k in ("dx", "d_o", "dqkv", "ln_partial"):
        assert torch.equal(bw[k], bw32[k]), f"attention lattice {kind} (B {B}, S {S}): float32 and float64 emulations differ in {k}"
    stats = dict(sums=sums, ctx_max=float(fw["ctx"].abs().max()), pre_max=float(fw["pre"].abs().max()), dx_max=float(bw["dx"].abs().max()),
                 dq_nonzero=int((bw["dqkv"][:, :E] != 0).sum()), dk_nonzero=int((bw["dqkv"][:, E:2 * E] != 0).sum()),
                 dv_nonzero=int((bw["dqkv"][:, 2 * E:] != 0).sum()))
    ops.update(keep_attn=ka, keep_ln=kl)
    return ops, fw, bops, bw, stats


def attn_random(B: int, S: int, seed: int, p: float = 0.0, seeds=(0, 0), word: int = 0, n_slab: int = 0):
    """the random case at the model's magnitudes: x, dy ~ N(0, 1), xavier-sized weights rounded to bf16, LayerNorm parameters near (1, 0),
    slabs ~ N(0, 1 / 4).  The backward's kept operands pre / mean / rstd are the plain forward's, rounded to fp32 (inputs of the launcher).
    -> (forward operands, backward operands, plain dict, emu32 dict, emu64 dict); each dict holds forward and backward tensors"""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    T = B * S
    f32 = lambda t: t.float().double()
    ops = dict(x=f32(n(T, E)), Wqkv=bf(u(3 * E, E) * (6.0 / (4 * E)) ** 0.5 * 1.5), bqkv=f32(n(3 * E) * 0.1), Wo=bf(u(E, E) * E ** -0.5), bo=f32(n(E) * 0.1),
               gamma=f32(1 + 0.1 * n(E)), beta=f32(0.1 * n(E)), eps=1e-5, B=B, S=S)
    ka, kl = attn_keep(p, seeds[0], seeds[1], word, B, S)
    out = []
    plain_f = attn_fwd(**ops, keep_attn=ka, keep_ln=kl)
    bops = dict(pre=f32(plain_f["pre"]), mean=f32(plain_f["mean"]), rstd=f32(plain_f["rstd"]), dy=f32(n(T, E)), slabs=f32(n(n_slab, T, E) * 0.5))
    common = dict(x=ops["x"], Wqkv=ops["Wqkv"], bqkv=ops["bqkv"], Wo=ops["Wo"], gamma=ops["gamma"], B=B, S=S, keep_attn=ka, keep_ln=kl)
    for acc, emu in ((torch.float64, False), (torch.float32, True), (torch.float64, True)):
        d = plain_f if not emu else attn_fwd(**ops, keep_attn=ka, keep_ln=kl, acc=acc, emulate=True)
        d = dict(d)
        d.update(attn_bwd(**common, **bops, acc=acc, emulate=emu))
        out.append(d)
    ops.update(keep_attn=ka, keep_ln=kl)
    return (ops, bops, *out)


def attn_rows(name: str, t: torch.Tensor, B: int) -> torch.Tensor:
    """the rows of kcheck.compare_rows: a token for activations and data gradients, a sequence for ln_partial and the LayerNorm statistics"""
    return t.reshape(B, -1) if name in ("ln_partial", "mean", "rstd") else t.reshape(-1, t.shape[-1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole trunk   dropout(emb + pos[pos_ids]) -> L post-norm layers -> mean over the sequence   (csrc/txl_block.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
LAYER_PARAMS = ("Wqkv", "bqkv", "Wo", "bo", "W1", "b1", "W2", "b2", "g1", "be1", "g2", "be2")
TRUNK_KEPT = ("y1", "pre1", "mean1", "rstd1", "ctx", "y2", "pre2", "mean2", "rstd2")          # per layer, what backward reads
TRUNK_BWD = ("d_o", "dqkv", "df", "h", "dh", "lnp1", "lnp2")                                  # per layer, what backward leaves


def trunk_seeds(site: int, L: int):
    """the layers' four dropout sites, as hulc2_amd/functional.py derives them from a call's site (oracle/counter_rng.py layer_site)"""
    return [dict(seed_attn=R.layer_site(site, l, R.ATTN), seed_ln1=R.layer_site(site, l, R.OUT), seed_ffn=R.layer_site(site, l, R.FFN),
                 seed_ln2=R.layer_site(site, l, R.LIN2)) for l in range(L)]


def trunk_keep(p: float, site: int, word: int, B: int, S: int, FF: int, L: int, b0: int = 0):
    """every keep-scale of one trunk launch for sequences b0 .. b0 + B - 1: pos (B S, E) and per layer attn, ln1, ffn, ln2"""
    one = lambda *s: torch.ones(*s, dtype=torch.float64)
    if p <= 0.0:
        return dict(pos=one(B * S, E), layers=[dict(attn=one(B, NH, S, S), ln1=one(B * S, E), ffn=one(B * S, FF), ln2=one(B * S, E)) for _ in range(L)])
    m = R.trunk_masks(p, site, word, B, S, E, NH, FF, L, row0=b0)
    t = lambda a, *shape: torch.from_numpy(a.astype(np.float64)).reshape(*shape)
    return dict(pos=t(m[R.POS], B * S, E),
                layers=[dict(attn=t(l[R.ATTN], B, NH, S, S), ln1=t(l[R.OUT], B * S, E), ffn=t(l[R.FFN], B * S, FF), ln2=t(l[R.LIN2], B * S, E))
                        for l in m["layers"]])


def trunk(emb, pos, pos_ids, layers, keep, dpooled, eps=1e-5, acc=torch.float64, emulate=False, fwd_emulate=None):
    """emb (B, S, E), pos (rows, E), pos_ids (S,) long, layers: list of dicts of LAYER_PARAMS, keep: trunk_keep(), dpooled (B, E).
    emulate: the kernels' bf16 rounding points (attn_fwd / attn_bwd / ffn) with `acc` arithmetic; fwd_emulate (default = emulate) sets the
    forward's separately: the split-operand forward has fp32-class operands while the backward stays on bf16.
    -> dict: x0 (T, E), pooled (B, E), demb (B, S, E), layers = list of dicts of TRUNK_KEPT + TRUNK_BWD (float64)"""
    fe = emulate if fwd_emulate is None else fwd_emulate
    B, S, _ = emb.shape
    c = lambda t: t.to(acc)
    x = ((c(emb) + c(pos)[pos_ids][None]).reshape(B * S, E) * c(keep["pos"]))
    out = dict(x0=x.double(), layers=[])
    kept = []
    for l, k in zip(layers, keep["layers"]):
        fw = attn_fwd(x, l["Wqkv"], l["bqkv"], l["Wo"], l["bo"], l["g1"], l["be1"], eps, B, S, k["attn"], k["ln1"], acc=acc, emulate=fe)
        y1 = c(fw["y"])
        f = ffn(y1, l["W1"], l["b1"], l["W2"], l["b2"], torch.zeros_like(y1), k["ffn"], acc=acc, emulate=fe)["f"]
        pre2 = y1 + c(f) * c(k["ln2"])
        mean2 = pre2.mean(-1)
        rstd2 = torch.rsqrt(((pre2 - mean2[:, None]) ** 2).mean(-1) + eps)
        y2 = (pre2 - mean2[:, None]) * rstd2[:, None] * c(l["g2"]) + c(l["be2"])
        kept.append(dict(x=x, y1=y1, pre1=c(fw["pre"]), mean1=c(fw["mean"]), rstd1=c(fw["rstd"]), ctx=c(fw["ctx"]), y2=y2, pre2=pre2, mean2=mean2, rstd2=rstd2))
        x = y2
    out["pooled"] = x.reshape(B, S, E).mean(1).double()
    dy = (c(dpooled) / S)[:, None, :].expand(B, S, E).reshape(B * S, E)
    bwd = [None] * len(layers)
    for li in range(len(layers) - 1, -1, -1):
        l, k, t = layers[li], keep["layers"][li], kept[li]
        dpre2, lnp2 = ln_bwd(dy, t["pre2"], t["mean2"], t["rstd2"], c(l["g2"]), B)
        r = bf if emulate else _ident
        fb = ffn(t["y1"], l["W1"], l["b1"], l["W2"], l["b2"], dpre2 * c(k["ln2"]), k["ffn"], acc=acc, emulate=emulate)
        dy1 = dpre2 + c(fb["dx"])
        bw = attn_bwd(t["x"], l["Wqkv"], l["bqkv"], l["Wo"], l["g1"], B, S, k["attn"], k["ln1"], t["pre1"], t["mean1"], t["rstd1"], dy1, acc=acc, emulate=emulate)
        bwd[li] = dict(d_o=bw["d_o"], dqkv=bw["dqkv"], df=r(dpre2 * c(k["ln2"])), h=fb["h"], dh=fb["dh"], lnp1=bw["ln_partial"], lnp2=lnp2)
        dy = c(bw["dx"])
    out["demb"] = (dy * c(keep["pos"])).reshape(B, S, E).double()
    for t, b in zip(kept, bwd):
        d = {n: t[n].double() for n in TRUNK_KEPT}
        d.update({n: b[n].double() for n in TRUNK_BWD})
        out["layers"].append(d)
    return out


def trunk_rows(t: torch.Tensor, B: int) -> torch.Tensor:
    """the rows of kcheck.compare_rows for every trunk tensor: a sequence"""
    return t.reshape(B, -1)


def trunk_pos_ids(S: int) -> torch.Tensor:
    """a non-monotonic sequence of table rows with a repeat (the table has 40 rows)"""
    ids = (torch.arange(S) * 7 + 3) % 37
    if S > 1:
        ids[S - 1] = ids[0]
    return ids


def trunk_random(B: int, S: int, L: int, FF: int, seed: int, p: float, site: int, word: int, ops_only: bool = False):
    """the random case at the model's magnitudes -> (operands dict, plain, emu32, emu64); ops_only: the operands alone (None for the rest)"""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    f32 = lambda t: t.float().double()
    layers = [_random_layer(g, FF) for _ in range(L)]
    ops = dict(emb=f32(n(B, S, E)), pos=f32(n(40, E) * 0.5), pos_ids=trunk_pos_ids(S), layers=layers, dpooled=f32(n(B, E)))
    if ops_only:
        return ops, None, None, None
    keep = trunk_keep(p, site, word, B, S, FF, L)
    plain = trunk(**ops, keep=keep)
    e32 = trunk(**ops, keep=keep, acc=torch.float32, emulate=True)
    e64 = trunk(**ops, keep=keep, acc=torch.float64, emulate=True)
    ops["keep"] = keep
    return ops, plain, e32, e64


def _random_layer(g, FF):
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    f32 = lambda t: t.float().double()
    return dict(Wqkv=bf(u(3 * E, E) * (6.0 / (4 * E)) ** 0.5 * 1.5), bqkv=f32(n(3 * E) * 0.1), Wo=bf(u(E, E) * E ** -0.5), bo=f32(n(E) * 0.1),
                W1=bf(u(FF, E) * E ** -0.5), b1=f32(u(FF) * 0.1), W2=bf(u(E, FF) * FF ** -0.5), b2=f32(u(E) * 0.1),
                g1=f32(1 + 0.1 * n(E)), be1=f32(0.1 * n(E)), g2=f32(1 + 0.1 * n(E)), be2=f32(0.1 * n(E)))


def trunk_lattice(B: int, S: int, L: int, FF: int, seed: int, site: int, word: int):
    """what composes exactly: integer emb and position table with dropout 0.5 give an exact layers[0].x for any S; with S = 1 (the one
    probability is 1) and integer attention weights in layer 0, that layer's ctx and pre1 are exact too.  Everything behind a LayerNorm is
    not on a lattice; those parameters are random.  -> (operands, exact dict x0 [, ctx, pre1])"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    layers = [_random_layer(g, FF) for _ in range(L)]
    layers[0].update(Wqkv=torch.cat([ri(-1, 1, 2 * E, E), ri(-2, 2, E, E)], 0), bqkv=ri(-3, 3, 3 * E), Wo=ri(-1, 1, E, E), bo=ri(-3, 3, E))
    ops = dict(emb=ri(-4, 4, B, S, E), pos=ri(-4, 4, 40, E), pos_ids=trunk_pos_ids(S), layers=layers,
               dpooled=torch.randn(B, E, generator=g, dtype=torch.float64).float().double())
    keep = trunk_keep(0.5, site, word, B, S, FF, L)
    x0 = (ops["emb"] + ops["pos"][ops["pos_ids"]][None]).reshape(B * S, E) * keep["pos"]
    exact = dict(x0=x0)
    if S == 1:
        l, k, sums = layers[0], keep["layers"][0], {}

        def check(name, a, b, extra=None):
            sums[name] = _assert_exact(f"trunk {name} (B {B})", a, b, extra)

        args = (x0, l["Wqkv"], l["bqkv"], l["Wo"], l["bo"], l["g1"], l["be1"], 1e-5, B, S, k["attn"], k["ln1"])
        fw = attn_fwd(*args, acc=torch.float64, emulate=True, check=check)
        fw32 = attn_fwd(*args, acc=torch.float32, emulate=True)
        for n in ("ctx", "pre"):
            assert torch.equal(fw[n], fw32[n]), f"trunk lattice (B {B}): float32 and float64 emulations differ in {n}"
        exact.update(ctx=fw["ctx"], pre1=fw["pre"])
    ops["keep"] = keep
    return ops, exact


def split_weights(w64: torch.Tensor):
    """an fp32 weight as the split-operand forward holds it: hi = bf16(w), lo = bf16(w - hi) -> (hi, lo) float64"""
    w = w64.float()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return hi.double(), lo.double()


def trunk_split(B: int, S: int, L: int, FF: int, seed: int, site: int, word: int, p: float = 0.0):
    """the split-operand forward: fp32 weights handed over as bf16 hi + lo pairs; both operands of every product enter with 16 mantissa bits.
    The reference is the plain float64 forward on the weights hi + lo; the yardstick is the same forward in float32 arithmetic (a
    float32-operand emulation).  -> (operands with layers[i][name + "_hi" / "_lo"], plain, emu32)"""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    layers = []
    for _ in range(L):
        l = _random_layer(g, FF)
        for name, scale in (("Wqkv", (6.0 / (4 * E)) ** 0.5 * 1.5), ("Wo", E ** -0.5), ("W1", E ** -0.5), ("W2", FF ** -0.5)):
            w = (torch.rand(l[name].shape, generator=g, dtype=torch.float64) * 2 - 1) * scale
            hi, lo = split_weights(w)
            l[name + "_hi"], l[name + "_lo"], l[name] = hi, lo, hi + lo
        layers.append(l)
    f32 = lambda t: t.float().double()
    ops = dict(emb=f32(n(B, S, E)), pos=f32(n(40, E) * 0.5), pos_ids=trunk_pos_ids(S), layers=layers, dpooled=torch.zeros(B, E, dtype=torch.float64))
    keep = trunk_keep(p, site, word, B, S, FF, L)
    plain = trunk(**ops, keep=keep)
    e32 = trunk(**ops, keep=keep, acc=torch.float32)
    ops["keep"] = keep
    return ops, plain, e32


def trunk_tensors(d: dict):
    """(name, tensor) of everything a trunk result holds"""
    yield "x0", d["x0"]
    yield "pooled", d["pooled"]
    yield "demb", d["demb"]
    for li, l in enumerate(d["layers"]):
        for n in TRUNK_KEPT + TRUNK_BWD:
            yield f"{li}.{n}", l[n]


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of the GPU files (tests/test_seqref_cpu.py walks the same lists)
# ---------------------------------------------------------------------------------------------------------------------------------
RNG_WORD = 0x2545F4914F6CDD1D            # a device RNG word with bits set in both halves (kernels.reset_step_state), as tests/test_dropout_gpu.py
FFN_SEED = 0x5EED0D0D                    # the site seed handed to hulc_ffn_fwd / hulc_ffn_bwd

FFN_LATTICE_T = (1, 63, 64, 65, 130, 16 * 64 + 5, 17 * 64 + 1)       # token groups walk 1 and 2 tiles, unevenly
FFN_LATTICE_FF = (128, 384, 2048)
FFN_RANDOM_CASES = [(T, FF, p) for T in (100, 1100, 2560) for FF in (384, 2048) for p in (0.0, 0.1)]
RNN_LATTICE_CASES = [(B, S) for B in (1, 7, 8, 33, 64) for S in (1, 2, 8)]
RNN_RANDOM_CASES = [(1, 1), (33, 3), (64, 8)]                          # (B, S)


def ffn_rows(name: str, t: torch.Tensor) -> torch.Tensor:
    """the rows of kcheck.compare_rows: a token for f / dx and their slice partials, an output feature for dW1 / dW2, all of db1"""
    return t.reshape(1, -1) if name == "db1" else t.reshape(-1, t.shape[-1])


def ffn_lattice_case(T: int, FF: int, p: float):
    return ffn_lattice(T, FF, seed=1000 * FF + T, p=p, rng_seed=FFN_SEED, word=RNG_WORD, big=True)


def ffn_random_case(T: int, FF: int, p: float):
    return ffn_random(T, FF, seed=7000 + T + FF, p=p, rng_seed=FFN_SEED, word=RNG_WORD)


def rnn_lattice_case(B: int, S: int, backward: bool):
    return rnn_lattice(S, B, seed=100 * B + S, backward=backward, amp=12 if backward else 40)


def rnn_random_case(B: int, S: int, backward: bool):
    return rnn_random(S, B, seed=300 + 10 * B + S, backward=backward)


ATTN_SEEDS = (0x5EED0A77, 0x5EED0111)                                  # seed_attn, seed_ln
ATTN_LATTICE_CASES = ([("single", B, 1) for B in (1, 3, 64)] + [("uniform", B, S) for B in (1, 3, 64) for S in (1, 2, 8, 32)]
                      + [("perm", B, S) for B in (1, 3, 64) for S in (3, 7, 8, 31, 32)])
ATTN_SLABS = (0, 1, 4, 5, 16)
ATTN_RANDOM_CASES = [(B, S, p, n) for (B, S) in ((1, 1), (3, 7), (5, 32), (64, 31)) for p in (0.0, 0.1) for n in (0, 16)]
ATTN_OUTPUTS = ("y", "pre", "mean", "rstd", "ctx", "dx", "d_o", "dqkv", "ln_partial")


def attn_lattice_slabs(B: int, S: int, p: float) -> int:
    """the number of partial slabs a lattice case's backward sums: every value of ATTN_SLABS comes up over the case list"""
    return ATTN_SLABS[(B + S + int(p > 0)) % len(ATTN_SLABS)]


def attn_lattice_case(kind: str, B: int, S: int, p: float, n_slab: int):
    return attn_lattice(B, S, kind, seed=50 * B + S, p=p, seeds=ATTN_SEEDS, word=RNG_WORD, n_slab=n_slab, backward=not (kind == "uniform" and S > 8))


def attn_random_case(B: int, S: int, p: float, n_slab: int):
    return attn_random(B, S, seed=900 + 40 * B + S, p=p, seeds=ATTN_SEEDS, word=RNG_WORD, n_slab=n_slab)


TRUNK_SITE = 0x5EED0001
TRUNK_RANDOM_CASES = [(64, 32, 2, 2048), (100, 19, 2, 2048), (130, 32, 1, 2048), (8, 32, 4, 256), (5, 7, 2, 384), (3, 32, 2, 128)]     # Q = 4, 2, 1, 2, 1, 1
TRUNK_SHARE = dict(zip(TRUNK_RANDOM_CASES, (4, 2, 1, 2, 1, 1)))
TRUNK_P = 0.1


def trunk_random_case(B: int, S: int, L: int, FF: int):
    return trunk_random(B, S, L, FF, seed=31 * B + S + L + FF, p=TRUNK_P, site=TRUNK_SITE, word=RNG_WORD)

TRUNK_SPLIT_CASES = [(8, 32, 4, 256), (5, 7, 2, 384)]


def trunk_split_case(B: int, S: int, L: int, FF: int):
    return trunk_split(B, S, L, FF, seed=77 * B + S, site=TRUNK_SITE, word=RNG_WORD)
