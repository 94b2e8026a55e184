"""CPU references of the MLP chain (csrc/mlp_chain.hip) and of the camera encoders' head (csrc/mlp2_rows.hip), used by
tests/test_mlp_chain_kernel_gpu.py and tests/test_mlp2_rows_kernel_gpu.py and checked on the CPU by tests/test_mlpref_cpu.py.  float64 torch
only: no GPU, no kernel code.

Unlike the feed-forward reference of tests/seqref.py, the bf16 rounding of a layer's INPUT is part of what these kernels define (the header
states it: the first stage rounds x0 to bf16, layers exchange bf16), so the float64 reference carries the rounding points itself:
  * `chain_layer_ref` / `mlp2_ref`: the kernel's rounding points, every product accumulated in float64;
  * `chain_layer_emu32` / `mlp2_ref(acc=torch.float32)`: the same rounding points with float32 accumulation (torch's CPU summation order).
    Its error against the float64 reference is the yardstick `e_ref` of kcheck.compare_rows: pure fp32 summation-order noise.  The
    float64-accumulating emulation IS the reference (it scores 0 x e_ref, tests/test_mlpref_cpu.py asserts that);
  * lattice builders: operands for which the builder asserts in float64 that every term of every accumulation is a multiple of one unit u
    and sum |terms| < 2^24 u, so that fp32 arithmetic in ANY order is exact, every rounding point rounds an exactly known value (round to
    nearest even, which .to(torch.bfloat16) reproduces) and the float64 reference is what the kernel must give BIT FOR BIT.

A chain case is a dict: M, K0, x0 (M, K0) float64 holding fp32 values, layers = [dict(W (N, K) float64 holding bf16 values, W_lo the same or
None, bias (N,) or None, relu, mask (M, N) or None, mask_scale)], x3 (split operands: every layer carries W_lo)."""
import torch

EXACT = float(2 ** 24)
KSW_SET = (1, 2, 3, 4, 8, 16, 32)


def bf(t: torch.Tensor) -> torch.Tensor:
    """round to bf16 (nearest even), keep the dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def split(t64: torch.Tensor):
    """hi = bf16(v), lo = bf16(v - hi) of fp32 values held in float64 (v - hi is exact in fp32, so float64 forms the same difference)"""
    hi = bf(t64)
    return hi, bf(t64 - hi)


def gran(t: torch.Tensor) -> float:
    """the largest power of two of which every element of t is a multiple (inf for an all-zero tensor)"""
    nz = t.double()[t != 0]
    if nz.numel() == 0:
        return float("inf")
    m, e = torch.frexp(nz)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()
    return 2.0 ** float((torch.log2(low) + e - 53).min())


def assert_exact_sum(what: str, products, extra=None) -> float:
    """the lattice condition of sum over (a, b) in products of a @ b^T (+ extra), all into ONE fp32 accumulator: with u the smallest unit of
    any term, sum |terms| < 2^24 u for every output element.  Returns the largest sum in units of u."""
    s, u = 0.0, float("inf")
    for a, b in products:
        s = s + a.double().abs() @ b.double().abs().t()
        u = min(u, gran(a) * gran(b))
    if extra is not None:
        s = s + extra.double().abs()
        u = min(u, gran(extra))
    if not torch.is_tensor(s) or not s.any():
        return 0.0
    m = float(s.max()) / u
    assert m < EXACT, f"lattice {what}: sum |terms| reaches {m:.0f} units >= 2^24, fp32 accumulation is no longer exact"
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# one layer of the chain, as csrc/mlp_chain.hip defines it
# ---------------------------------------------------------------------------------------------------------------------------------
def _chain_layer(a_prev64, W, bias, relu, mask, mask_scale, x3, W_lo, acc, check=None):
    a = a_prev64.double()
    hi, lo = split(a)
    c = lambda t: t.to(acc)
    Wa = c(W)
    products = [(hi, W)]
    if x3:                                                          # a_hi w_hi + a_lo w_hi + a_hi w_lo, no lo x lo term
        products += [(lo, W), (hi, W_lo)]
    if x3 and acc == torch.float32:
        # the mode is DEFINED with one fp32 accumulator that takes all three products of a k-step (of 32), k-step after k-step: the small
        # lo products are rounded at the accumulator's full magnitude.  Three separate float32 GEMMs added at the end (a third of those
        # roundings) are no float32 evaluation of that definition — measured on an MI355X, K = 2048: kernel 4.3e-07, three GEMMs 1.6e-07,
        # this 4.1e-07, chain_layer_tree32(group=8) 4.2e-07 with 89 % of the kernel's bits reproduced.  Plain k order, no wave split.
        v = torch.zeros(a.shape[0], W.shape[0], dtype=torch.float32)
        for k0 in range(0, W.shape[1], 32):
            for p, q in products:
                v = (v.double() + p[:, k0:k0 + 32] @ q[:, k0:k0 + 32].t()).float()
    elif x3:
        v = c(hi) @ Wa.t() + c(lo) @ Wa.t() + c(hi) @ c(W_lo).t()
    else:
        v = c(hi) @ Wa.t()
    if check is not None:
        check(products, None if bias is None else bias.expand(a.shape[0], -1))
    if bias is not None:
        v = v + c(bias)
    if mask is not None:                                            # the mask wins over relu
        v = torch.where(mask > 0, v * torch.tensor(float(torch.tensor(mask_scale, dtype=torch.float32)), dtype=acc), torch.zeros((), dtype=acc))
    elif relu:
        v = v.clamp_min(0.0)
    return v.double()


def chain_layer_ref(a_prev64, W, bias=None, relu=False, mask=None, mask_scale=1.0, x3=False, W_lo=None):
    """one layer in float64: the input rounded to bf16 (chain_stage_input / the exchange store), the product with the bf16 weights, + bias,
    then mask > 0 ? v * mask_scale : 0 when a mask is given, else ReLU when `relu`; x3: hi / lo operands, three products"""
    return _chain_layer(a_prev64, W, bias, relu, mask, mask_scale, x3, W_lo, torch.float64)


def chain_layer_emu32(a_prev64, W, bias=None, relu=False, mask=None, mask_scale=1.0, x3=False, W_lo=None):
    """the same rounding points with float32 accumulation, bias add and mask scaling: the yardstick of kcheck.compare_rows (plain: torch's
    float32 GEMM; x3: one float32 accumulator over the k-steps, as the mode is defined — see _chain_layer)"""
    return _chain_layer(a_prev64, W, bias, relu, mask, mask_scale, x3, W_lo, torch.float32)


def chain_layer_tree32(a_prev64, W, bias=None, relu=False, mask=None, mask_scale=1.0, x3=False, W_lo=None, group=32):
    """float32 emulation in the KERNEL's summation order (chain_layer<KSW>): wave w of 4 owns the k-steps (of 32) w KSW .. w KSW + KSW - 1
    of K padded up to 128 KSW and adds them one after the other into its accumulator — x3: a_hi w_hi, a_lo w_hi, a_hi w_lo per k-step into
    the SAME accumulator — then (w0 + w1) + (w2 + w3), + bias, epilogue.  group: k-terms that enter the accumulator with one fp32 rounding
    (32: one rounding per MFMA instruction; each group's dot product is taken exactly, in float64).  Not a yardstick: the explanation of
    what a ratio of tests/test_mlp_chain_kernel_gpu.py measures.  Measured on an MI355X (random (1000, (2048, 16)) and (40, (48, 16))
    chains, 17 rows, plain and split operands): group = 8 — the 16x16x32 bf16 MFMA adds the four 8-wide k-blocks of its lane groups one
    after the other, rounding each time — reproduces 89 % .. 100 % of the kernel's output bits and its error to 3 %; group = 32, 16 and 4
    reproduce 6 % .. 60 % of the bits of the 2048-deep layers.  So a k-step costs 4 roundings at the accumulator's magnitude (12 with split
    operands), which is why the kernel scores up to 1.5 x the float32 GEMM of the CPU and scored 2.78 x three separate ones."""
    a = a_prev64.double()
    hi, lo = split(a)
    K = W.shape[1]
    ksw = ksw_of(K)
    pad = lambda t: torch.nn.functional.pad(t.double(), (0, ksw * 128 - K))
    pairs = [(pad(hi), pad(W))] + ([(pad(lo), pad(W)), (pad(hi), pad(W_lo))] if x3 else [])
    part = []
    for w in range(4):
        acc = torch.zeros(a.shape[0], W.shape[0], dtype=torch.float32)
        for s in range(ksw):
            k0 = (w * ksw + s) * 32
            for p, q in pairs:
                for g0 in range(k0, k0 + 32, group):
                    acc = (acc.double() + p[:, g0:g0 + group] @ q[:, g0:g0 + group].t()).float()
        part.append(acc)
    v = (part[0] + part[1]) + (part[2] + part[3])
    if bias is not None:
        v = v + bias.float()
    if mask is not None:
        v = torch.where(mask > 0, v * torch.tensor(mask_scale, dtype=torch.float32), torch.zeros((), dtype=torch.float32))
    elif relu:
        v = v.clamp_min(0.0)
    return v.double()


def _layer_args(case, lay):
    return dict(W=lay["W"], bias=lay["bias"], relu=lay["relu"], mask=lay["mask"], mask_scale=lay["mask_scale"], x3=case["x3"], W_lo=lay["W_lo"])


def chain_free(case, layer_fn=chain_layer_ref):
    """free-running: layer l is fed the reference's own output of layer l - 1 -> list of (M, N_l) float64"""
    outs, a = [], case["x0"]
    for lay in case["layers"]:
        a = layer_fn(a, **_layer_args(case, lay))
        outs.append(a)
    return outs


def chain_forced(case, fed, layer_fn=chain_layer_ref):
    """teacher-forced: layer l is fed fed[l - 1], the caller-visible fp32 output of layer l - 1 of the run under test (the kernel packs its
    exchange copy from the registers it stores to `out`), rounded as the kernel rounds it -> list of (M, N_l) float64"""
    outs = []
    for l, lay in enumerate(case["layers"]):
        a = case["x0"] if l == 0 else fed[l - 1].detach().double().cpu()
        outs.append(layer_fn(a, **_layer_args(case, lay)))
    return outs


def chain_widths(case):
    return [lay["W"].shape[0] for lay in case["layers"]]


def ksw_of(K: int) -> int:
    return (K + 127) // 128


def k_slot(k: int, ksw: int):
    """(wave, k-step, 8-group) that column k of a layer's input falls to in chain_layer<KSW>"""
    return (k // 32) // ksw, (k // 32) % ksw, (k % 32) // 8


def _layer(W, W_lo=None, bias=None, relu=False, mask=None, mask_scale=1.0):
    return dict(W=W, W_lo=W_lo, bias=bias, relu=bool(relu), mask=mask, mask_scale=float(mask_scale))


def _case(M, K0, x0, layers, x3=False):
    k = K0
    for lay in layers:
        assert lay["W"].shape[1] == k and torch.equal(bf(lay["W"]), lay["W"]) and (lay["W_lo"] is not None) == x3
        k = lay["W"].shape[0]
    assert x0.shape == (M, K0) and torch.equal(x0.float().double(), x0)
    return dict(M=M, K0=K0, x0=x0, layers=layers, x3=x3)


def _distinct_rows_cols(t, what):
    if t.shape[0] > 1:
        assert torch.unique(t, dim=0).shape[0] == t.shape[0], f"{what}: two rows are equal"


# ---------------------------------------------------------------------------------------------------------------------------------
# lattices of the chain
# ---------------------------------------------------------------------------------------------------------------------------------
def perm_chain(M: int, K0: int, widths, seed: int, amp: int = 128):
    """permutation chain: W_l has a single 1.0 per row at k = pi_l(n); pi_l (seeded) maps into [0, K) and hits every (wave, k-step, 8-group)
    of the layer's k range (asserted).  A layer with fewer rows than 8-groups (N < K / 8: a narrow layer behind a wide one) cannot do that
    with one entry per row: its rows carry ceil(K / 8 / N) ones, one per group, and its outputs are sums of that many relocated values.
    x[m][k] = ((a_m k + c_m) mod (2 amp + 1)) - amp with a row-specific odd multiplier: signed integers of magnitude <= amp, different per
    row, distinct within any window of 2 amp + 1 columns.  No bias, no ReLU: the outputs are relocated input values and any slip in the
    blocked layout, the MFMA lane map or the row / tile ownership moves a value.  Asserts that every exchanged activation is exact in bf16
    (amp <= 128, or smaller where sums are exchanged)."""
    g = torch.Generator().manual_seed(seed)
    mod = 2 * amp + 1
    k = torch.arange(K0, dtype=torch.int64)
    rows = []
    for m in range(M):
        a_m, c_m = 2 * ((7 * m + seed) % amp) + 1, (37 * m + 11 * seed) % mod
        rows.append(((a_m * k + c_m) % mod - amp).double())
    x0 = torch.stack(rows)
    layers, K = [], K0
    for l, N in enumerate(widths):
        groups = K // 8
        per_row = -(-groups // N)
        W = torch.zeros(N, K, dtype=torch.float64)
        # every group once (shuffled over the rows), the remaining slots drawn at random; the column inside the group at random
        slots = torch.cat([torch.randperm(groups, generator=g), torch.randint(0, groups, (N * per_row - groups,), generator=g)])
        slots = slots[torch.randperm(slots.numel(), generator=g)] if per_row == 1 else slots
        slots = slots.view(per_row, N)
        for j in range(per_row):
            cols = slots[j] * 8 + torch.randint(0, 8, (N,), generator=g)
            W[torch.arange(N), cols] = 1.0
        seen = {k_slot(int(c), ksw_of(K)) for c in W.nonzero()[:, 1]}
        assert len(seen) == groups, f"permutation chain layer {l} (K {K}, N {N}): {len(seen)} of {groups} (wave, k-step, group) slots hit"
        assert int((W != 0).sum(1).max()) <= per_row and int((W != 0).sum(1).min()) >= 1
        layers.append(_layer(W))
        K = N
    case = _case(M, K0, x0, layers)
    _distinct_rows_cols(x0, "permutation chain x0")
    assert_lattice(case)
    return case


def dense_chain(M: int, K0: int, widths, seed: int, nnz: int = 4, bias: bool = True, relu="alt", masks: bool = False, x3: bool = False,
                last_random: bool = False, amp: int = 3, bamp: int = 2):
    """dense lattice: weights in {-1, 0, 1} * 2^-s with `nnz` non-zeros per row spread over the four waves' k ranges (where the layer's k
    range reaches them), s = l % 3, integer inputs in [-amp, amp], biases = integers in [-bamp, bamp] in units of the layer's lattice; relu: "alt"
    (on for even layers), True or False; masks: every layer carries a mask with zeros, negatives and positives and mask_scale 1.25 (relu
    also set: the mask must win).  x3: inputs integer + {-1, 0, 1} * 2^-10 (a non-zero lo part that is exact), W_lo in {-1, 0, 1} * 2^-10
    (layer 0) / 2^-6 (later layers).  last_random: the LAST layer gets continuous nn.Linear-style weights and bias (the hidden activations
    stay on the lattice: a free-running reference without bf16 flips).  Asserts the 2^24 condition of every accumulation and that every
    exchanged activation is exact in bf16 (x3: in its hi + lo pair)."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    x0 = ri(-amp, amp, M, K0)
    for _ in range(100):                                             # no two rows equal
        if torch.unique(x0, dim=0).shape[0] == M:
            break
        x0 = ri(-amp, amp, M, K0)
    if x3:
        x0 = torch.where(x0 == 0, torch.ones_like(x0), x0) + ri(-1, 1, M, K0) * 2.0 ** -10
    layers, K, unit = [], K0, 1.0
    for l, N in enumerate(widths):
        last = l + 1 == len(widths)
        ksw = ksw_of(K)
        if last and last_random:
            W = bf((torch.rand(N, K, generator=g, dtype=torch.float64) * 2 - 1) * K ** -0.5)
            W_lo = None
            b = ((torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * K ** -0.5).float().double()
        else:
            s = l % 3
            W = torch.zeros(N, K, dtype=torch.float64)
            n_nz = min(nnz, K)
            for n in range(N):
                cols = set()
                for w in range(4):                                   # one non-zero in each wave's k range that exists
                    lo_k, hi_k = w * ksw * 32, min((w + 1) * ksw * 32, K)
                    if lo_k < hi_k and len(cols) < n_nz:
                        cols.add(int(torch.randint(lo_k, hi_k, (1,), generator=g)))
                while len(cols) < n_nz:
                    cols.add(int(torch.randint(0, K, (1,), generator=g)))
                cols = torch.tensor(sorted(cols))
                W[n, cols] = (ri(0, 1, len(cols)) * 2 - 1) * 2.0 ** -s
            W_lo = None
            if x3:
                W_lo = torch.zeros(N, K, dtype=torch.float64)
                pick = torch.rand(N, K, generator=g) < min(1.0, 4.0 / K)
                W_lo[pick] = ((ri(0, 1, int(pick.sum())) * 2 - 1) * 2.0 ** (-10 if l == 0 else -6))
            unit *= 2.0 ** -s
            b = ri(-bamp, bamp, N) * unit if bias else None
        if isinstance(relu, str):
            r = l % 2 == 0
        else:
            r = bool(relu)
        mask = None
        if masks:
            mask = ri(-2, 2, M, N) * 0.5                             # zeros, negatives and positives
            mask[:, 0] = (torch.arange(M, dtype=torch.float64) % 3) - 1
        layers.append(_layer(W, W_lo, b, r or masks, mask, 1.25 if masks else 1.0))
        K = N
    case = _case(M, K0, x0, layers, x3)
    _distinct_rows_cols(x0, "dense lattice x0")
    assert_lattice(case, skip_last=last_random)
    return case


def assert_lattice(case, skip_last: bool = False):
    """the exactness claims of a lattice case, in float64: every accumulation satisfies sum |terms| < 2^24 units, the mask scaling is exact
    in fp32, every exchanged activation is exact in bf16 (x3: hi + lo reproduces it), the float32-accumulating emulation gives the float64
    reference's bits, and so does a float32 accumulation over the REVERSED k order.  Returns the free-running reference outputs."""
    outs, a = [], case["x0"]
    nl = len(case["layers"])
    for l, lay in enumerate(case["layers"]):
        args = _layer_args(case, lay)
        exact = not (skip_last and l + 1 == nl)
        what = f"chain layer {l} (M {case['M']}, K {lay['W'].shape[1]}, N {lay['W'].shape[0]})"
        chk = (lambda products, extra: assert_exact_sum(what, products, extra)) if exact else None
        v = _chain_layer(a, acc=torch.float64, check=chk, **args)
        if exact:
            assert torch.equal(v.float().double(), v), f"{what}: the output is not an fp32 number"
            v32 = chain_layer_emu32(a, **args)
            assert torch.equal(v32, v), f"{what}: float32 and float64 accumulation differ"
            rev = dict(args, W=lay["W"].flip(1), W_lo=None if lay["W_lo"] is None else lay["W_lo"].flip(1))
            assert torch.equal(chain_layer_emu32(a.flip(1), **rev), v), f"{what}: float32 accumulation in reversed k order differs"
        if l + 1 < nl:
            hi, lo = split(v)
            back = hi + lo if case["x3"] else hi
            assert torch.equal(back, v), f"{what}: {int((back != v).sum())} exchanged activations are not exact in bf16"
        outs.append(v)
        a = v
    return outs


def random_chain(M: int, K0: int, widths, seed: int, masks: bool = False, x3: bool = False):
    """model magnitudes: nn.Linear initialisation (uniform in +-1 / sqrt(K), weights rounded to bf16 — x3: to their hi + lo pair — biases
    to fp32), randn inputs rounded to fp32; ReLU on every layer but the last; masks: randn masks with mask_scale 1.25 on every layer"""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(M, K0, generator=g, dtype=torch.float64).float().double()
    layers, K = [], K0
    for l, N in enumerate(widths):
        w = ((torch.rand(N, K, generator=g, dtype=torch.float64) * 2 - 1) * K ** -0.5).float().double()
        W, W_lo = split(w)
        b = ((torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * K ** -0.5).float().double()
        mask = torch.randn(M, N, generator=g, dtype=torch.float64).float().double() if masks else None
        layers.append(_layer(W, W_lo if x3 else None, b, l + 1 < len(widths), mask, 1.25 if masks else 1.0))
        K = N
    return _case(M, K0, x0, layers, x3)


# the shapes of tests/test_mlp_chain_kernel_gpu.py: every KSW instance runs as layer 0 (the staged input) and as a later layer (an exchange
# region); the two 4096 cases are kept to one lattice and one random case each
CHAIN_M = (1, 5, 16, 17, 33, 48, 63, 64)
CHAIN_PAIRS = ((1, 32), (32, 1), (5, 17), (16, 16), (32, 32))
CHAIN_SHAPES = [(8, (16,)), (40, (48, 16)), (136, (256, 144, 16)), (264, (384, 32)), (392, (512, 1024, 16)), (1000, (2048, 16)),
                (24, (64, 16, 48, 32, 16, 64, 32, 16))]
CHAIN_SHAPES_4096 = [(2040, (4096, 16)), (4096, (16, 16))]


MASK_KW = dict(nnz=2, amp=1, bamp=1)         # dense lattices with masks: mask_scale 1.25 costs 2.3 bits per layer
DEEP_KW = dict(nnz=2, amp=1, bamp=1)         # ... and of more than 3 layers: 1 bit per layer


def perm_amp(K0, widths) -> int:
    """amplitude of a permutation chain's inputs: 128, or less where a narrow layer that is exchanged sums several relocated values"""
    amp, K = 128, K0
    for l, N in enumerate(widths[:-1]):
        per_row = -(-(K // 8) // N)
        amp = min(amp, 256 // per_row) if per_row > 1 else amp
        K = N
    return amp


def ksw_coverage(shapes):
    """{KSW: (runs as layer 0, runs as a later layer)} over a list of (K0, widths)"""
    seen = {}
    for K0, widths in shapes:
        K = K0
        for l in range(len(widths)):
            a, b = seen.get(ksw_of(K), (False, False))
            seen[ksw_of(K)] = (a or l == 0, b or l > 0)
            K = widths[l]
    return seen


# ---------------------------------------------------------------------------------------------------------------------------------
# the head fc2(relu(fc1(x))) and its backward, as csrc/mlp2_rows.hip defines them
# ---------------------------------------------------------------------------------------------------------------------------------
def mlp2_ref(x, W1, b1, W2, b2, dy, x3=False, W1_lo=None, W2_lo=None, acc=torch.float64, check=None, dh_fed=None, full=False):
    """x (T, 128), W1 (H, 128), b1 (H), W2 (OUT, H), b2 (OUT), dy (T, OUT): float64 tensors holding storage values (x, b, dy fp32; W bf16).
    The kernel's rounding points: x -> bf16; the hidden tile relu(z) -> bf16 as the operand of the second product; dy -> bf16;
    dh = (W2^T dy) * gate -> bf16, stored and reused as the operand of dx.  x3 (forward only): both products from hi / lo splits of both
    operands, without the lo x lo term; the backward always recomputes the hidden tile from bf16 operands.
    dh_fed: teacher-forced dx, the product of the dh the run under test STORED (bf16 values) instead of the reference's own rounding.
    -> y (forward, x3 as given), h, dh, dx (plain backward), all float64; full: also the hidden tile and dh BEFORE their bf16 rounding
    (what a bf16 output is compared with, half an ulp allowed: kcheck.half_ulp)"""
    c = lambda t: t.to(acc)
    check = check or (lambda *a: None)
    xh, xl = split(x.double())
    W1a, W2a = c(W1), c(W2)
    z = c(xh) @ W1a.t() + c(b1)
    check("z", [(xh, W1)], b1.expand(x.shape[0], -1))
    gate = z > 0
    h_full = torch.where(gate, z, torch.zeros((), dtype=acc))
    h = bf(h_full)
    if x3:
        check("z x3", [(xh, W1), (xl, W1), (xh, W1_lo)], b1.expand(x.shape[0], -1))
        z3 = c(xh) @ W1a.t() + c(xl) @ W1a.t() + c(xh) @ c(W1_lo).t() + c(b1)
        hh, hl = split(z3.clamp_min(0.0).double())
        check("y x3", [(hh, W2), (hl, W2), (hh, W2_lo)], b2.expand(x.shape[0], -1))
        y = c(hh) @ W2a.t() + c(hl) @ W2a.t() + c(hh) @ c(W2_lo).t() + c(b2)
    else:
        check("y", [(h, W2)], b2.expand(x.shape[0], -1))
        y = h @ W2a.t() + c(b2)
    dyb = bf(c(dy))
    check("dh", [(dyb, W2.t())])
    dh_full = torch.where(gate, dyb @ W2a, torch.zeros((), dtype=acc))
    dh = bf(dh_full) if dh_fed is None else c(dh_fed.double())
    check("dx", [(dh, W1.t())])
    dx = dh @ W1a
    out = (y.double(), h.double(), dh.double(), dx.double())
    return out + (h_full.double(), dh_full.double()) if full else out


MLP2_T = (1, 31, 32, 33, 65, 96)
MLP2_H = (128, 384)
MLP2_OUT = (32, 64, 96, 128)


def _sparse_rows(g, N, K, nnz, lo, hi):
    """(N, K) with nnz entries per row, the first four in the hidden units of the four waves (wave w owns units 32 w .. 32 w + 31 of every
    128), integers in [lo, hi] \\ 0"""
    W = torch.zeros(N, K, dtype=torch.float64)
    for n in range(N):
        cols = [int(torch.randint(0, K // 128, (1,), generator=g)) * 128 + 32 * q + int(torch.randint(0, 32, (1,), generator=g)) for q in range(4)]
        cols += [int(c) for c in torch.randint(0, K, (max(nnz - 4, 0),), generator=g)]
        v = torch.randint(lo, hi + 1, (len(cols),), generator=g).double()
        W[n, torch.tensor(cols)] = torch.where(v == 0, torch.ones_like(v), v)
    return W


def mlp2_lattice(T: int, H: int, OUT: int, seed: int, x3: bool = False):
    """integer operands for which y, h, dh and dx are exact: x in [-7, 7], W1 in [-3, 3] (x3: [-4, 4], [-2, 2]), b1 in [-8, 8], W2 in [-1, 1], b2 in [-3, 3],
    dy in [-3, 3]; hidden values above 256 exercise the bf16 rounding of h and dh.  x3: x = non-zero integer + {-1, 0, 1} * 2^-10 (a
    non-zero lo part that is exact), W1_lo in {-1, 0, 1} * 2^-10, W2 sparse (8 non-zeros per row over all four waves' hidden units) and W2_lo
    in {-1, 0, 1} * 2^-2, so that the three-product sums stay inside 24 bits.  Asserts the 2^24 condition of every accumulation and that
    float32 accumulation, in two orders, gives the float64 reference's bits.  -> (operands dict, (y, h, dh, dx))"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    xa, wa = (4, 2) if x3 else (7, 3)
    ops = dict(x=ri(-xa, xa, T, 128), W1=ri(-wa, wa, H, 128), b1=ri(-8, 8, H), W2=ri(-1, 1, OUT, H), b2=ri(-3, 3, OUT), dy=ri(-3, 3, T, OUT))
    ops["x"][:, 0] = torch.arange(T, dtype=torch.float64) % 9 - 4
    lo = {}
    if x3:
        ops["x"] = torch.where(ops["x"] == 0, torch.ones_like(ops["x"]), ops["x"]) + ri(-1, 1, T, 128) * 2.0 ** -10
        ops["W2"] = _sparse_rows(g, OUT, H, 8, -1, 1)
        lo = dict(W1_lo=ri(-1, 1, H, 128) * 2.0 ** -10, W2_lo=(ops["W2"] != 0) * ri(-1, 1, OUT, H) * 2.0 ** -2)
    what = f"mlp2 lattice (T {T}, H {H}, OUT {OUT}, x3 {x3})"
    want = mlp2_ref(**ops, x3=x3, **lo, check=lambda name, products, extra=None: assert_exact_sum(f"{what} {name}", products, extra))
    w32 = mlp2_ref(**ops, x3=x3, **lo, acc=torch.float32)
    flip = dict(ops, x=ops["x"].flip(1), W1=ops["W1"].flip(1))
    flo = dict(lo, W1_lo=lo["W1_lo"].flip(1)) if x3 else {}
    r32 = mlp2_ref(**flip, x3=x3, **flo, acc=torch.float32)
    for name, a, b, c in zip(("y", "h", "dh", "dx"), want, w32, r32):
        assert torch.equal(a.float().double(), a), f"{what}: {name} is not an fp32 number"
        assert torch.equal(a, b), f"{what}: float32 and float64 accumulation differ in {name}"
        if name != "dx":                                            # (dx of the flipped problem is the flipped dx)
            assert torch.equal(a, c), f"{what}: float32 accumulation over the reversed input order differs in {name}"
        else:
            assert torch.equal(a, c.flip(1)), f"{what}: float32 accumulation over the reversed input order differs in dx"
    ops.update(lo)
    return ops, want


def mlp2_random(T: int, H: int, OUT: int, seed: int, x3: bool = False):
    """model magnitudes with the pre-activation on a dyadic grid (x: multiples of 2^-4 in [-2, 2], W1: multiples of 2^-6 in [-1/8, 1/8],
    b1: multiples of 2^-10 in [-1/8, 1/8]; x3: x is non-zero and carries an extra {0, 1} * 2^-12 away from zero, W1_lo is a multiple of 2^-14), so that z is exact
    in fp32 and neither a ReLU gate nor the hidden tile's bf16 rounding can differ between kernel and reference (asserted); W2 (x3: its
    hi + lo pair), b2 and dy are continuous.  -> (operands dict, ref64 = (y, h, dh, dx, h and dh before rounding), emu32 = the same with float32 accumulation)"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    ops = dict(x=torch.round(u(T, 128) * 32) / 16, W1=torch.round(u(H, 128) * 8) / 64, b1=torch.round(u(H) * 128) / 1024)
    w2 = (u(OUT, H) * H ** -0.5).float().double()
    W2, W2_lo = split(w2)
    ops.update(W2=W2, b2=(u(OUT) * 0.1).float().double(), dy=u(T, OUT).float().double())
    assert torch.equal(ops["x"], bf(ops["x"])) and torch.equal(ops["W1"], bf(ops["W1"]))
    lo = {}
    if x3:
        ops["x"] = torch.where(ops["x"] == 0, torch.full_like(ops["x"], 2.0 ** -4), ops["x"])
        ops["x"] = ops["x"] + torch.sign(ops["x"]) * torch.round(u(T, 128).abs()) * 2.0 ** -12      # (away from zero: bf16(x) stays on the 2^-4 grid)
        lo = dict(W1_lo=torch.round(u(H, 128) * 4) * 2.0 ** -14, W2_lo=W2_lo)
        assert torch.equal(bf(lo["W1_lo"]), lo["W1_lo"]) and torch.equal(ops["x"].float().double(), ops["x"])
    ref = mlp2_ref(**ops, x3=x3, **lo, full=True)
    e32 = mlp2_ref(**ops, x3=x3, **lo, acc=torch.float32, full=True)
    exact = []
    mlp2_ref(**ops, x3=x3, **lo, check=lambda name, products, extra=None: exact.append(assert_exact_sum(f"mlp2 random {name}", products, extra))
             if name.startswith("z") else None)
    assert torch.equal(ref[1], e32[1]), "the dyadic pre-activation is not exact in fp32: a gate or a rounding of h could differ"
    ops.update(lo)
    return ops, ref, e32


def mlp2_seed(T, H, OUT, x3=False) -> int:
    return 1000 * T + H + OUT + (7 if x3 else 0)
