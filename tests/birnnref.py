"""CPU references of the BiRNN plan-recognition posterior: the paired recurrent sweep of csrc/rnn_wavefront.hip (hulc_rnn_wavefront_pair)
as include/hulc2_amd.h states it, its lattice and random case builders, and the module's float64 forward and backward.  Used by
tests/test_birnn_cpu.py, tests/test_rnn_pair_kernel_gpu.py and tests/test_birnn_gpu.py; the conventions (plain float64 reference, rounding-point
emulation with `acc` / `emulate`, lattice builders that assert the 2^24 condition) are those of tests/seqref.py."""
import torch

from tests import seqref as Q
from tests.seqref import bf

H = 2048


# ---------------------------------------------------------------------------------------------------------------------------------
# paired sweep
# ---------------------------------------------------------------------------------------------------------------------------------
def pair_sweep(S, B, H, wA, wB2, add1=None, add1c=None, add2=None, add2c=None, bias1=(None, None), bias2=(None, None), mask1=None, mask2=None,
               relu=False, acc=torch.float64, emulate=False, check=None, lag=False):
    """State rows z[0 .. S] (S + 1, B, 2H) in SWEEP order.  wA, wB2 (H, H): element (n, k) multiplies input k of output n.  add1, add2, mask1,
    mask2 are indexed by wave step, (S, B, H) each; add1c, add2c are (B, H).  Row 0 is zero; wave step tau = 0 .. S-1 writes row tau + 1:
          first half:   f1(z_tau[:, :H] wA^T  + add1[tau] + add1c + bias1a + bias1b)
          second half:  f2(z_tau[:, H:] wB2^T + add2[tau] + add2c + bias2a + bias2b)
    f keeps where mask[tau] > 0 when a mask is given, else ReLU when relu.  wB2 None is the solo sweep: the second half stays zero.
    emulate / acc: as seqref.rnn_sweep (the state is rounded to bf16 once per wave step as the next step's operand).
    lag=True puts the decoder sweep's one-step lag back (S + 1 wave steps, rows 0 .. S+1, the first half written for tau < S, the second for
    tau >= 1, add2 / mask2 indexed 0 .. S): seqref.rnn_sweep with wB1 = 0, which tests/test_birnn_cpu.py asserts bit for bit."""
    c = lambda t: None if t is None else t.to(acc)
    check = check or (lambda *a: None)
    wA, wB2, add1, add1c, add2, add2c, mask1, mask2 = map(c, (wA, wB2, add1, add1c, add2, add2c, mask1, mask2))
    zero = torch.zeros(H, dtype=acc)
    b1 = sum((c(b) for b in bias1 if b is not None), zero)
    b2 = sum((c(b) for b in bias2 if b is not None), zero)
    if add1c is not None:
        b1 = b1 + add1c
    if add2c is not None:
        b2 = b2 + add2c
    steps = S + 1 if lag else S
    z = torch.zeros(steps + 1, B, 2 * H, dtype=acc)
    gate = lambda v, m, tau: torch.where(m[tau] > 0, v, torch.zeros_like(v)) if m is not None else (v.clamp_min(0) if relu else v)
    for tau in range(steps):
        zin = bf(z[tau]) if emulate else z[tau]
        if tau < S:
            e = b1 + (add1[tau] if add1 is not None else 0)
            check(f"first[{tau}]", zin[:, :H], wA.t(), e.expand(B, H))
            z[tau + 1, :, :H] = gate(zin[:, :H] @ wA.t() + e, mask1, tau)
        if wB2 is not None and (tau >= 1 or not lag):
            e = b2 + (add2[tau] if add2 is not None else 0)
            check(f"second[{tau}]", zin[:, H:], wB2.t(), e.expand(B, H))
            z[tau + 1, :, H:] = gate(zin[:, H:] @ wB2.t() + e, mask2, tau)
    return z.double()


def pair_lattice(S: int, B: int, seed: int, backward: bool, H: int = H, nnz: int = 3, amp: int = 3):
    """integer operands of one paired sweep, as seqref.rnn_lattice builds the decoder's.  Forward mode: relu, integer add1 / add2 in
    [-amp, amp], add1c / add2c in [-2, 2], four small negative biases.  Backward mode: masks in {-1, 0, 0.5, 3}, integer add1 / add2, no
    biases.  The two halves draw independent data (a swapped or un-reversed half cannot pass).  Asserts the 2^24 condition at every wave
    step and that the float32 and float64 emulations agree bit for bit.  -> (operands for pair_sweep, expected rows (S + 1, B, 2H), stats)"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    ops = dict(wA=Q.sparse_sign_matrix(H, g, nnz), wB2=Q.sparse_sign_matrix(H, g, nnz), add1=ri(-amp, amp, S, B, H), add2=ri(-amp, amp, S, B, H))
    if backward:
        vals = torch.tensor([-1.0, 0.0, 0.5, 3.0], dtype=torch.float64)
        ops.update(mask1=vals[torch.randint(0, 4, (S, B, H), generator=g)], mask2=vals[torch.randint(0, 4, (S, B, H), generator=g)], relu=False)
    else:
        ops.update(add1c=ri(-2, 2, B, H), add2c=ri(-2, 2, B, H), bias1=(ri(-1, 0, H), ri(-1, 0, H)), bias2=(ri(-1, 0, H), ri(-1, 0, H)), relu=True)
    sums = []

    def check(name, a, b, extra=None):
        sums.append(Q._assert_exact(f"pair {name} (S {S}, B {B})", a, b, extra))

    want = pair_sweep(S, B, H, **ops, acc=torch.float64, emulate=True, check=check)
    w32 = pair_sweep(S, B, H, **ops, acc=torch.float32, emulate=True)
    assert torch.equal(want, w32), f"pair lattice (S {S}, B {B}): float32 and float64 emulations differ"
    a = want.abs()
    stats = dict(sum_max=max(sums), z_max=float(a.max()), nonzero=float((want[1:] != 0).double().mean()), rounded=int((bf(want) != want).sum()))
    return ops, want, stats


def pair_random(S: int, B: int, seed: int, backward: bool, H: int = H):
    """the random case at the model's magnitudes (seqref.rnn_random's distributions, both halves with external terms of their own).
    -> (operands, plain float64 rows, emu32 rows, emu64 rows)"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()
    k = H ** -0.5
    w = lambda: (u(H, H) * k).to(torch.bfloat16).double()
    ops = dict(wA=w(), wB2=w(), add1=n(S, B, H), add2=n(S, B, H))
    if backward:
        ops.update(mask1=n(S, B, H), mask2=n(S, B, H), relu=False)
    else:
        b = lambda: (u(H) * k).float().double()
        ops.update(add1c=n(B, H), add2c=n(B, H), bias1=(b(), b()), bias2=(b(), b()), relu=True)
    plain = pair_sweep(S, B, H, **ops)
    e32 = pair_sweep(S, B, H, **ops, acc=torch.float32, emulate=True)
    e64 = pair_sweep(S, B, H, **ops, acc=torch.float64, emulate=True)
    return ops, plain, e32, e64


def pair_rows(z: torch.Tensor) -> torch.Tensor:
    """the rows of kcheck.compare_rows for a paired sweep's state rows in sweep order: (wave step, batch row, half) of rows 1 .. S -> (n, H)"""
    Sp1, B, H2 = z.shape
    h = H2 // 2
    return torch.cat([z[1:, :, :h].reshape(-1, h), z[1:, :, h:].reshape(-1, h)], 0)


PAIR_LATTICE_CASES = [(1, 1), (7, 2), (8, 8), (33, 3), (64, 8)]        # (B, S): one row, a row-group tail, 8 rows, the second row half, the full tile
PAIR_RANDOM_CASES = [(1, 1), (33, 3), (64, 8)]


def pair_lattice_case(B: int, S: int, backward: bool):
    return pair_lattice(S, B, seed=500 + 100 * B + S, backward=backward, amp=12 if backward else 40)


def pair_random_case(B: int, S: int, backward: bool):
    return pair_random(S, B, seed=700 + 10 * B + S, backward=backward)


# ---------------------------------------------------------------------------------------------------------------------------------
# the module: nn.RNN(in, 2048, num_layers=2, nonlinearity="relu", bidirectional=True, batch_first=True), out[:, -1], then fc_state
# ---------------------------------------------------------------------------------------------------------------------------------
RNN_KEYS = [f"birnn_model.{n}_l{l}{r}" for l in (0, 1) for r in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def module_shapes(in_features: int = 128, state_out: int = 1024, hidden: int = H) -> dict:
    """name -> shape of the 18 parameters of PlanRecognitionBiRNNNetwork (state_out = plan_features, or 2 * plan_features for the Gaussian)"""
    s = {}
    for l in (0, 1):
        k = in_features if l == 0 else 2 * hidden
        for r in ("", "_reverse"):
            s[f"birnn_model.weight_ih_l{l}{r}"] = (hidden, k)
            s[f"birnn_model.weight_hh_l{l}{r}"] = (hidden, hidden)
            s[f"birnn_model.bias_ih_l{l}{r}"] = (hidden,)
            s[f"birnn_model.bias_hh_l{l}{r}"] = (hidden,)
    s["fc_state.0.weight"] = (state_out, 2 * hidden)
    s["fc_state.0.bias"] = (state_out,)
    return s


def _direction(x, w_ih, w_hh, b_ih, b_hh, reverse):
    """one direction of one layer: x (B, S, K) -> (B, S, hidden), h_t = relu(x_t w_ih^T + b_ih + h_prev w_hh^T + b_hh)"""
    B, S, _ = x.shape
    h = x.new_zeros(B, w_hh.shape[0])
    out = [None] * S
    for t in (range(S - 1, -1, -1) if reverse else range(S)):
        h = torch.relu(x[:, t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh)
        out[t] = h
    return torch.stack(out, 1)


def module_forward(params: dict, emb: torch.Tensor):
    """params: the 18 tensors by state-dict name (any float dtype), emb (B, S, in_features) -> (state (B, state_out), x (B, 2 * hidden)):
    the arithmetic of the module in the dtype of its inputs, built from differentiable torch operations"""
    p = lambda n: params["birnn_model." + n]
    x = emb
    for l in (0, 1):
        f = _direction(x, p(f"weight_ih_l{l}"), p(f"weight_hh_l{l}"), p(f"bias_ih_l{l}"), p(f"bias_hh_l{l}"), False)
        b = _direction(x, p(f"weight_ih_l{l}_reverse"), p(f"weight_hh_l{l}_reverse"), p(f"bias_ih_l{l}_reverse"), p(f"bias_hh_l{l}_reverse"), True)
        x = torch.cat([f, b], -1)
    last = x[:, -1]
    return last @ params["fc_state.0.weight"].t() + params["fc_state.0.bias"], last


def module_backward(params: dict, emb: torch.Tensor, g_state: torch.Tensor, g_x: torch.Tensor):
    """float64 forward and backward: -> (state, x, {name: gradient} for the 18 parameters and "emb")"""
    leaves = {k: v.detach().double().requires_grad_(True) for k, v in params.items()}
    e = emb.detach().double().requires_grad_(True)
    state, x = module_forward(leaves, e)
    (state * g_state.double()).sum().add((x * g_x.double()).sum()).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    grads["emb"] = e.grad
    return state.detach(), x.detach(), grads


def module_params(seed: int, in_features: int = 128, state_out: int = 1024, hidden: int = H) -> dict:
    """a seeded fill at nn.RNN's own initial magnitudes, U(-1, 1) / sqrt(hidden) (fc_state: / sqrt(2 * hidden)); float32 values"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in module_shapes(in_features, state_out, hidden).items():
        k = (2 * hidden if name.startswith("fc_state") else hidden) ** -0.5
        out[name] = ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * k).float()
    return out


def module_case(seed: int, B: int, S: int, in_features: int = 128, state_out: int = 1024, hidden: int = H):
    """-> (params, emb (B, S, in_features), cotangents of state and x): everything float32-representable"""
    g = torch.Generator().manual_seed(seed + 1)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
    return module_params(seed, in_features, state_out, hidden), n(B, S, in_features), n(B, state_out), n(B, 2 * hidden) * 0.1


def module_emulated(params: dict, emb, g_state, g_x, acc=torch.float32, emulate: bool = True):
    """The module's forward and backward written out the way functional.BiRNNPosteriorFn computes them, with its rounding points: every GEMM
    operand (weights, activations, deltas) rounded to bf16 when `emulate`, products accumulated in `acc`, the recurrences through pair_sweep
    (state rounded once per wave step).  emulate=False, acc=float64 is module_backward (tests/test_birnn_cpu.py); emulate=True, acc=float32
    is the yardstick e_ref of the bf16 module tests.  -> (state, x, {name: gradient} with "emb")"""
    r = bf if emulate else (lambda t: t)
    c = lambda t: t.detach().to(acc)
    P = lambda n: c(params["birnn_model." + n])
    B, S, E = emb.shape
    Hh = P("weight_hh_l0").shape[0]
    mm = lambda a, w: r(a) @ r(w).t()                                   # a (.., K), w (N, K)
    kw = dict(acc=acc, emulate=emulate)
    emb_t = c(emb).transpose(0, 1)                                      # (S, B, E)
    pre_f = mm(emb_t, P("weight_ih_l0")) + P("bias_ih_l0")
    pre_b = mm(emb_t, P("weight_ih_l0_reverse")) + P("bias_ih_l0_reverse")
    z0 = pair_sweep(S, B, Hh, r(P("weight_hh_l0")), r(P("weight_hh_l0_reverse")), add1=pre_f, add2=pre_b.flip(0), bias1=(P("bias_hh_l0"), None),
                    bias2=(P("bias_hh_l0_reverse"), None), relu=True, **kw).to(acc)
    hf0, hb0 = z0[1:, :, :Hh], z0[1:, :, Hh:].flip(0)                    # time order
    x1 = torch.cat([hf0, hb0], -1)
    u = mm(x1, P("weight_ih_l1")) + P("bias_ih_l1")
    hf1 = pair_sweep(S, B, Hh, r(P("weight_hh_l1")), None, add1=u, bias1=(P("bias_hh_l1"), None), relu=True, **kw).to(acc)[1:, :, :Hh]
    hb1 = torch.relu(mm(x1[S - 1], P("weight_ih_l1_reverse")) + (P("bias_ih_l1_reverse") + P("bias_hh_l1_reverse")))
    x = torch.cat([hf1[S - 1], hb1], -1)
    wfc, gs = c(params["fc_state.0.weight"]), c(g_state)
    state = mm(x, wfc) + c(params["fc_state.0.bias"])
    # backward
    g = c(g_x) + r(gs) @ r(wfc)
    gr = {"fc_state.0.weight": r(gs).t() @ r(x), "fc_state.0.bias": gs.sum(0)}
    db1 = torch.where(hb1 > 0, g[:, Hh:], torch.zeros_like(hb1))
    g1 = torch.zeros(S, B, Hh, dtype=acc)
    g1[0] = g[:, :Hh]                                                   # wave step 0 is t = S-1
    d1 = pair_sweep(S, B, Hh, r(P("weight_hh_l1")).t(), None, add1=g1, mask1=hf1.flip(0), **kw).to(acc)[1:, :, :Hh].flip(0)
    dx1 = r(d1) @ r(P("weight_ih_l1"))
    dx1[S - 1] += r(db1) @ r(P("weight_ih_l1_reverse"))
    d0 = pair_sweep(S, B, Hh, r(P("weight_hh_l0")).t(), r(P("weight_hh_l0_reverse")).t(), add1=dx1[:, :, :Hh].flip(0), mask1=hf0.flip(0),
                    add2=dx1[:, :, Hh:], mask2=hb0, **kw).to(acc)
    df0, db0 = d0[1:, :, :Hh].flip(0), d0[1:, :, Hh:]
    tok = lambda a: r(a).reshape(-1, a.shape[-1])
    gw = lambda d, z: tok(d).t() @ tok(z)
    zero = torch.zeros(1, B, Hh, dtype=acc)
    n = "birnn_model."
    gr.update({n + "weight_ih_l1": gw(d1, x1), n + "bias_ih_l1": tok(d1).sum(0), n + "weight_hh_l1": gw(d1, torch.cat([zero, hf1[:-1]])),
               n + "bias_hh_l1": tok(d1).sum(0), n + "weight_ih_l1_reverse": r(db1).t() @ r(x1[S - 1]), n + "bias_ih_l1_reverse": db1.sum(0),
               n + "weight_hh_l1_reverse": torch.zeros(Hh, Hh, dtype=acc), n + "bias_hh_l1_reverse": db1.sum(0),
               n + "weight_hh_l0": gw(df0, torch.cat([zero, hf0[:-1]])), n + "bias_hh_l0": tok(df0).sum(0),
               n + "weight_hh_l0_reverse": gw(db0, torch.cat([hb0[1:], zero])), n + "bias_hh_l0_reverse": tok(db0).sum(0),
               n + "weight_ih_l0": gw(df0, emb_t), n + "bias_ih_l0": tok(df0).sum(0),
               n + "weight_ih_l0_reverse": gw(db0, emb_t), n + "bias_ih_l0_reverse": tok(db0).sum(0),
               "emb": (r(df0) @ r(P("weight_ih_l0")) + r(db0) @ r(P("weight_ih_l0_reverse"))).transpose(0, 1)})
    return state.double(), x.double(), {k: v.double() for k, v in gr.items()}
