"""CPU references of the decoder RNN's inter-layer dropout (policy_rnn_dropout_p; csrc/rnn_wavefront.hip: hulc_rnn_wavefront_drop,
hulc_rnn_drop_rows), used by tests/test_rnn_dropout_cpu.py, tests/test_rnn_dropout_kernel_gpu.py and tests/test_rnn_dropout_gpu.py.

  * mask builders: the convention of include/hulc2_amd.h, k_t[b][j] = dropout_scale(site ^ word, (t B + b) H + j, p), from the numpy twin
    of the device RNG (oracle/counter_rng.py), and torch's own time-major draw, replayed;
  * two_layer_rnn: the float64 restatement of nn.RNN(num_layers=2, nonlinearity="relu", dropout=p) as two one-layer recurrences with
    k_t * h0_t between them (autograd gives every gradient); tests/test_rnn_dropout_cpu.py pins it against torch's module;
  * sweep: seqref.rnn_sweep (the recurrence as the header states it) with the two masked modes of hulc_rnn_wavefront_drop, plain or with
    the kernel's rounding points, and the lattice / random cases built on seqref's operands.
"""
import numpy as np
import torch

from oracle import counter_rng as R
from tests import seqref as Q

DECODER_RNN_SITE = 0x5EED7001
MODALITY_SITES = {"vis": 0x5EED7101, "lang": 0x5EED7201}
MODE_K, MODE_N = 1, 2                    # HULC_RNN_DROP_K (forward sweep: the product's inputs), HULC_RNN_DROP_N (backward sweep: its outputs)


def keep_scales(p: float, site: int, word: int, S: int, B: int, H: int, row0: int = 0) -> torch.Tensor:
    """(S, B, H) float64 keep-scales in {0, fp32(1 / (1 - p))}: element (t, b, j) from index ((t B + b) + row0) H + j; all ones for p = 0"""
    if p <= 0.0:
        return torch.ones(S, B, H, dtype=torch.float64)
    idx = (np.arange(S * B * H, dtype=np.uint64) + np.uint64(row0 * H)).reshape(S, B, H)
    return torch.from_numpy(R.dropout_scale(int(site) ^ (int(word) & R.MASK64), idx, p).astype(np.float64))


def torch_mask(seed: int, p: float, S: int, B: int, H: int) -> torch.Tensor:
    """the mask nn.RNN(batch_first=True, dropout=p) draws between its two layers under torch.manual_seed(seed): ONE time-major draw,
    -> (S, B, H) float64 scales in {0, 1 / (1 - p)}"""
    torch.manual_seed(seed)
    return torch.dropout(torch.ones(S, B, H, dtype=torch.float64), p, True)


def two_layer_rnn(x, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1, keep=None):
    """x (B, S, I), keep (S, B, H) scales or None -> (h1 (B, S, H), h_n (2, B, H)), zero initial state.  Layer 0's recurrence, the output
    and h_n are undropped; only layer 1's input is k_t * h0_t."""
    B, S, _ = x.shape
    H = w_hh0.shape[0]
    h0, h1, out = x.new_zeros(B, H), x.new_zeros(B, H), []
    for t in range(S):
        h0 = torch.relu(x[:, t] @ w_ih0.t() + b_ih0 + h0 @ w_hh0.t() + b_hh0)
        inp = h0 if keep is None else h0 * keep[t].to(h0.dtype)
        h1 = torch.relu(inp @ w_ih1.t() + b_ih1 + h1 @ w_hh1.t() + b_hh1)
        out.append(h1)
    return torch.stack(out, 1), torch.stack([h0, h1])


def sweep(S, B, H, wA, wB1, wB2, keep, mode, add1=None, add1c=None, bias1=(None, None), bias2=(None, None), mask1=None, mask2=None,
          relu=False, acc=torch.float64, emulate=False, check=None):
    """seqref.rnn_sweep with the mask of hulc_rnn_wavefront_drop on the second half's wB1 product; keep (S, B, H) scales indexed by time step.
          MODE_K (t = tau - 1):  f2( s * ((keep01 . z_tau[:, :H]) wB1^T) + z_tau[:, H:] wB2^T + biases ),  s = fp32(1 / (1 - p)) applied in `acc`
          MODE_N (t = S - tau):  f2( keep_t . (z_tau[:, :H] wB1^T) + z_tau[:, H:] wB2^T + biases )
    The first half is rnn_sweep's.  emulate: the state is rounded to bf16 once per wave step (the zeroed values stay zero)."""
    c = lambda t: None if t is None else t.to(acc)
    check = check or (lambda *a: None)
    wA, wB1, wB2, add1, add1c, mask1, mask2, keep = map(c, (wA, wB1, wB2, add1, add1c, mask1, mask2, keep))
    zero = torch.zeros(H, dtype=acc)
    b1 = sum((c(b) for b in bias1 if b is not None), zero)
    b2 = sum((c(b) for b in bias2 if b is not None), zero)
    if add1c is not None:
        b1 = b1 + add1c
    s = keep.max()                                                    # the one non-zero value of the mask
    z = torch.zeros(S + 2, B, 2 * H, dtype=acc)
    for tau in range(S + 1):
        zin = Q.bf(z[tau]) if emulate else z[tau]
        if tau < S:
            e = b1 + (add1[tau] if add1 is not None else 0)
            check(f"first[{tau}]", zin[:, :H], wA.t(), e.expand(B, H))
            v = zin[:, :H] @ wA.t() + e
            v = torch.where(mask1[tau] > 0, v, torch.zeros_like(v)) if mask1 is not None else (v.clamp_min(0) if relu else v)
            z[tau + 1, :, :H] = v
        if tau >= 1:
            # (the bound of both modes: every term of the masked product at its full scale)
            check(f"second[{tau}]", torch.cat([s * zin[:, :H], zin[:, H:]], 1), torch.cat([wB1, wB2], 1).t(), b2.expand(B, H))
            if mode == MODE_K:
                k01 = (keep[tau - 1] > 0).to(acc)
                v = s * ((k01 * zin[:, :H]) @ wB1.t()) + zin[:, H:] @ wB2.t() + b2
            else:
                v = keep[S - tau] * (zin[:, :H] @ wB1.t()) + zin[:, H:] @ wB2.t() + b2
            v = torch.where(mask2[tau] > 0, v, torch.zeros_like(v)) if mask2 is not None else (v.clamp_min(0) if relu else v)
            z[tau + 1, :, H:] = v
    return z.double()


RNG_WORD = Q.RNG_WORD                    # a device RNG word with bits in both halves
LATTICE_CASES = [(1, 1), (7, 2), (8, 8), (33, 3), (64, 8)]               # (B, S): one row, a row-group tail, the mirror width, the second row half, the full tile
RANDOM_CASES = [(1, 1), (33, 3), (64, 8)]
LATTICE_P, RANDOM_P = 0.5, 0.1


def _mode(backward: bool) -> int:
    return MODE_N if backward else MODE_K


def lattice_case(B: int, S: int, backward: bool, H: int = 2048):
    """the operands of seqref.rnn_lattice_case (sparse +-1 weights, integer add terms) under the counter-RNG mask with p = 0.5, whose scale
    is 2: asserts the 2^24 condition at every wave step and that the float32 and float64 emulations agree bit for bit.
    -> (operands for seqref / the kernel, keep (S, B, H), expected rows (S + 2, B, 2H) float64)"""
    ops, _, _ = Q.rnn_lattice_case(B, S, backward)
    keep = keep_scales(LATTICE_P, DECODER_RNN_SITE, RNG_WORD, S, B, H)
    assert set(keep.unique().tolist()) <= {0.0, 2.0}

    def check(name, a, b, extra=None):
        Q._assert_exact(f"rnn dropout {name} (S {S}, B {B})", a, b, extra)

    want = sweep(S, B, H, **ops, keep=keep, mode=_mode(backward), acc=torch.float64, emulate=True, check=check)
    w32 = sweep(S, B, H, **ops, keep=keep, mode=_mode(backward), acc=torch.float32, emulate=True)
    assert torch.equal(want, w32), f"rnn dropout lattice (S {S}, B {B}): float32 and float64 emulations differ"
    return ops, keep, want


def random_case(B: int, S: int, backward: bool, H: int = 2048):
    """seqref's random operands at the model's magnitudes under the counter-RNG mask, p = 0.1
    -> (operands, keep, plain float64 rows, emulation rows with float32 accumulation)"""
    ops, _, _, _ = Q.rnn_random(S, B, seed=300 + 10 * B + S, backward=backward, H=H)
    keep = keep_scales(RANDOM_P, DECODER_RNN_SITE, RNG_WORD, S, B, H)
    plain = sweep(S, B, H, **ops, keep=keep, mode=_mode(backward))
    e32 = sweep(S, B, H, **ops, keep=keep, mode=_mode(backward), acc=torch.float32, emulate=True)
    return ops, keep, plain, e32
