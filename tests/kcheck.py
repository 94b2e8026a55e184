"""Shared pieces of the kernel-level tests (tests/test_reductions_gpu.py, tests/test_losses_gpu.py, tests/test_ffn_kernel_gpu.py,
tests/test_rnn_kernel_gpu.py, tests/test_conv_paths_gpu.py, tests/test_resnet_pieces_gpu.py, tests/test_lang_kernels_gpu.py,
tests/test_mlp_chain_kernel_gpu.py, tests/test_mlp2_rows_kernel_gpu.py, tests/test_grid_kernels_gpu.py).

Every case of those files follows one pattern:
  1. inputs are drawn on the CPU in float64 from a seeded generator and rounded to the kernel's storage type; the float64 reference is given
     the ROUNDED values, so only the kernel's arithmetic is measured;
  2. every output (and in/out operand) lives inside a larger allocation (`Guarded`) whose guard bands and padding columns hold a sentinel bit
     pattern that must be bit-identical after the call;
  3. the result is compared with the float64 reference under `compare()`;
  4. the call is repeated on the same inputs and must reproduce the bits (the kernels promise fixed summation orders);
  5. out-of-contract calls must raise through lib.check with the launcher's message and leave sentinel-filled outputs untouched (`refused()`).

The tolerance is not a number copied from what the kernels score.  For every compared tensor the test evaluates the SAME formula with torch
on the CPU in float32 and takes its error `e_ref` against the float64 reference in the same norm (max-abs over the tensor's max-abs for
activations and losses, relative L2 for gradients, as close() of tests/test_parity_gpu.py).  The bound is margin * max(e_ref, 2^-23); the
margin comes from the table at the top of each test file.  bf16 / fp16 outputs get half an ulp of the storage type on top, per element."""
import pytest
import torch

EPS32 = 2.0 ** -23
GUARD = 64                       # guard band in elements on either side (a multiple of 16 bytes for every type used here)
_SENTINEL = {torch.float32: (torch.int32, 0x7FC5A5A5),      # quiet NaNs with a recognisable payload: a stray read shows up as NaN
             torch.bfloat16: (torch.int16, 0x7FC5),
             torch.float16: (torch.int16, 0x7E5A),
             torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A),
             torch.int32: (torch.int32, 0x5A5A5A5A),
             torch.uint8: (torch.uint8, 0xA5)}

RATIOS = {}                      # kernel name -> largest (GPU error / max(e_ref, 2^-23)) seen, printed once per module


def rnd(t64: torch.Tensor, dtype) -> torch.Tensor:
    """float64 values rounded to the storage type, returned as float64 (what the reference is given)"""
    return t64.to(dtype).double()


def sentinel_full(n: int, dtype, dev) -> torch.Tensor:
    it, bits = _SENTINEL[dtype]
    return torch.full((n,), bits, dtype=it, device=dev).view(dtype)


class Guarded:
    """(rows, cols) block with row pitch ld >= cols inside a sentinel-filled allocation; `t` is the (rows, cols) view handed to the kernel
    (its data_ptr is the block's first element), `lead` extra elements shift the block (a misaligned view)."""

    def __init__(self, dev, rows, cols, dtype=torch.float32, ld=None, init=None, lead=0):
        ld = cols if ld is None else ld
        self.rows, self.cols, self.ld, self.g0 = rows, cols, ld, GUARD + lead
        n = rows * ld if rows else 0
        self.buf = sentinel_full(self.g0 + n + GUARD, dtype, dev)
        self.full = self.buf[self.g0:self.g0 + n].view(rows, ld)
        self.t = self.full[:, :cols]
        if init is not None:
            self.t.copy_(init.to(dtype).reshape(rows, cols))
        self._snap = self.buf.clone()
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)
        inside[self.g0:self.g0 + n].view(rows, ld)[:, :cols] = True
        self._outside = ~inside

    def assert_guards(self, what: str) -> None:
        it = _SENTINEL[self.buf.dtype][0]
        now, was = self.buf.view(it)[self._outside], self._snap.view(it)[self._outside]
        bad = int((now != was).sum())
        assert bad == 0, f"{what}: {bad} sentinel elements outside the ({self.rows}, {self.cols}) block (pitch {self.ld}) were overwritten"

    def assert_untouched(self, what: str) -> None:
        it = _SENTINEL[self.buf.dtype][0]
        assert torch.equal(self.buf.view(it), self._snap.view(it)), f"{what}: a refused call wrote to its output"

    def value(self) -> torch.Tensor:
        return self.t.detach().clone()


def out_flat(dev, n, dtype=torch.float32, init=None, lead=0) -> Guarded:
    return Guarded(dev, 1, n, dtype, init=init, lead=lead)


def half_ulp(ref64: torch.Tensor, dtype) -> torch.Tensor:
    """half a unit in the last place of `dtype` at each reference value (0 for float32 outputs: the bound already speaks float32)"""
    if dtype == torch.float32:
        return torch.zeros_like(ref64)
    mant, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    _, ex = torch.frexp(ref64.abs().clamp_min(2.0 ** emin))
    return torch.ldexp(torch.ones_like(ref64), (ex - 1 - mant).to(torch.int32))


def compare(kernel: str, what: str, got, ref64, ref32, margin: float, grad: bool = False, out_dtype=torch.float32) -> float:
    """assert `got` against the float64 reference under margin * max(e_ref, 2^-23) (+ half an ulp of a low-precision output type per element);
    returns and records the ratio error / max(e_ref, 2^-23)"""
    got = got.detach().double().cpu().reshape(-1)
    ref64 = ref64.detach().double().cpu().reshape(-1)
    ref32 = ref32.detach().double().cpu().reshape(-1)
    assert got.shape == ref64.shape == ref32.shape, f"{what}: shapes {tuple(got.shape)} / {tuple(ref64.shape)} / {tuple(ref32.shape)}"
    assert torch.isfinite(ref64).all(), f"{what}: the float64 reference is not finite (a broken test case)"
    assert torch.isfinite(got).all(), f"{what}: non-finite values from the kernel"
    excess = ((got - ref64).abs() - half_ulp(ref64, out_dtype)).clamp_min(0.0)
    if grad and got.numel() > 1:
        scale = ref64.norm().item()
        err, e_ref = excess.norm().item(), (ref32 - ref64).norm().item()
    else:
        scale = ref64.abs().max().item()
        err, e_ref = excess.max().item(), (ref32 - ref64).abs().max().item()
    if scale == 0.0:
        assert err == 0.0, f"{what}: the reference is exactly zero, the kernel left {err:.3e}"
        return 0.0
    err, e_ref = err / scale, e_ref / scale
    base = max(e_ref, EPS32)
    ratio = err / base
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    print(f"[kcheck] {kernel:28s} {what:12s} gpu {err:.3e}  cpu-f32 {e_ref:.3e}  ratio {ratio:.2f}  (margin {margin:g})")
    assert err <= margin * base, (f"{kernel} {what}: error {err:.3e} > {margin:g} * max(e_ref {e_ref:.3e}, 2^-23) "
                                  f"(ratio {ratio:.2f}; norm: {'relative L2' if grad else 'max-abs / max-abs'})")
    return ratio


def row_errors(got, ref64) -> torch.Tensor:
    """per row of a (rows, cols) pair: L2 norm of the difference over L2 norm of the reference row (float64)"""
    return (got - ref64).norm(dim=1) / ref64.norm(dim=1)


def compare_rows(kernel: str, what: str, got, ref64, emu32, margin: float) -> float:
    """compare() with a LOCALISED norm and an emulation as the yardstick: `got`, the float64 reference and the CPU rounding-point emulation
    with float32 accumulation are (rows, cols); the error is the maximum over rows of (row L2 error / row L2 norm of the reference) and the
    bound is margin * max(e_ref, 2^-23) with e_ref the emulation's error in the same norm.  A row is the unit a fault would hit (a token, a
    sequence, an output feature, a (wave step, batch row, half) of the recurrence): one wrong row fails however many right ones surround it.
    No row is excluded: a reference row that is exactly zero must come back exactly zero."""
    got = got.detach().double().cpu()
    ref64, emu32 = ref64.detach().double().cpu(), emu32.detach().double().cpu()
    assert got.dim() == 2 and got.shape == ref64.shape == emu32.shape, f"{what}: shapes {tuple(got.shape)} / {tuple(ref64.shape)} / {tuple(emu32.shape)}"
    assert torch.isfinite(ref64).all() and torch.isfinite(emu32).all(), f"{what}: the reference is not finite (a broken test case)"
    assert torch.isfinite(got).all(), f"{what}: non-finite values from the kernel"
    live = ref64.norm(dim=1) > 0
    assert not got[~live].any(), f"{what}: {int((~live).sum())} reference rows are exactly zero, the kernel left values there"
    assert live.any(), f"{what}: the reference is zero everywhere (a broken test case)"
    errs = row_errors(got[live], ref64[live])
    err, e_ref = errs.max().item(), row_errors(emu32[live], ref64[live]).max().item()
    base = max(e_ref, EPS32)
    ratio = err / base
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    worst = int(live.nonzero()[errs.argmax()])
    print(f"[kcheck] {kernel:28s} {what:12s} gpu {err:.3e}  cpu-emu32 {e_ref:.3e}  ratio {ratio:.2f}  (margin {margin:g}, worst row {worst} of {got.shape[0]})")
    assert err <= margin * base, (f"{kernel} {what}: error {err:.3e} > {margin:g} * max(e_ref {e_ref:.3e}, 2^-23) "
                                  f"(ratio {ratio:.2f}; norm: max over rows of relative L2, worst row {worst})")
    return ratio


def same_bits(a: torch.Tensor, b: torch.Tensor, what: str) -> None:
    assert torch.equal(a, b), f"{what}: a second call on the same inputs gave different bits (fixed summation order promised)"


def refused(call, message: str, *outputs: Guarded) -> None:
    """an out-of-contract call: raises HulcKernelError carrying the launcher's message, and the sentinel-filled outputs stay as they were"""
    from hulc2_amd.lib import HulcKernelError

    with pytest.raises(HulcKernelError) as ei:
        call()
    assert message in str(ei.value), f"expected the launcher's message {message!r}, got {ei.value}"
    torch.cuda.synchronize()
    for o in outputs:
        o.assert_untouched(message)


def report(title: str) -> None:
    print(f"\n[kcheck] largest GPU error / max(e_ref, 2^-23) per kernel — {title}")
    for k in sorted(RATIOS):
        print(f"[kcheck-max] {k:28s} {RATIOS[k]:8.2f}")
