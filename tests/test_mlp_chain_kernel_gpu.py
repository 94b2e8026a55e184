"""Kernel-level tests of csrc/mlp_chain.hip: kn.mlp_chain / kn.mlp_chain2 (and the C entry points with a workspace of the test's own) called
directly, against the float64 references of tests/mlpref.py.

  * exact cases, free-running: permutation chains (every output a relocated input value; every (wave, k-step, 8-group) slot of every layer
    hit) and dense lattices (sparse +-2^-s weights over all four waves' k ranges, integer inputs and biases) for which fp32 sums are exact
    in any order and every exchanged activation is exact in bf16: every layer's fp32 output must equal the float64 reference BIT FOR BIT.
    With and without bias, ReLU on and off per layer, the mask epilogue (zeros, negatives, positives, mask_scale 1.25, relu also set),
    pairs with different input widths both ways and a shorter second chain, split operands alone and as the second chain of a pair;
  * random cases at the model's magnitudes, TEACHER-FORCED per layer: the reference of layer l is fed the kernel's own caller-visible output
    of layer l - 1 (the kernel packs its exchange copy from the registers it stores to `out`), so kernel and reference differ in fp32
    summation order only, per row (kcheck.compare_rows) — and an exchange copy that disagrees with `out` fails in the next layer.  The
    last layer is also compared with a FREE-RUNNING reference on cases whose hidden activations sit on the lattice (no bf16 flips);
  * the workspace contract: exactly hulc_mlp_chain_workspace bytes inside guard bands, everything behind the header poisoned with bf16
    NaNs, the whole header zero after the launch, two different chains back to back on one workspace;
  * refusals (host-side checks that return before any launch).
Every operand has a row pitch wider than its logical width (x0 and masks are column slices of wider buffers, W a row slice with ldw > K,
outputs kcheck.Guarded with ld_out > N) inside sentinel NaNs.  The pattern of a case is that of tests/kcheck.py.

The total of a chain's exchange elements is 64 x the sum of its widths (multiples of 16), so it is never odd: the workspace cases take a
one-layer chain (no exchange region at all) and a pair with K0_b > K0_a (the blocked input is sized by the larger one) instead."""
import ctypes
import time

import pytest
import torch

from tests import kcheck as K
from tests import mlpref as R
from tests.kcheck import Guarded, compare_rows, refused, same_bits, sentinel_full

pytestmark = pytest.mark.gpu

# margin * max(e_ref, 2^-23) per tensor, e_ref = the CPU emulation of the same rounding points with float32 accumulation against float64,
# per row.  Kernel and emulation differ in fp32 summation order only: the project's standing margin for that is 2
# (tests/test_ffn_kernel_gpu.py).  Largest ratios measured on an MI355X ([kcheck-max] lines of this file):
#   mlp_chain 1.52   mlp_chain mask 1.03   mlp_chain x3 1.11   mlp_chain2 1.36   mlp_chain free 0.78
# A finding on the way: with three separate float32 GEMMs as the split-operand yardstick the 2048-deep layer of the random
# (1000, (2048, 16)) chain scored 2.78 (kernel 4.34e-07, yardstick 1.56e-07).  The kernel is right: mlpref.chain_layer_tree32, the CPU
# emulation of its 4-wave order with the MFMA adding its four 8-wide k-blocks one by one, reproduces 89 % of that layer's bits and its
# error (4.2e-07).  The mode puts three products per k-step into ONE accumulator, and the yardstick now does the same (mlpref._chain_layer).
MARGIN = 2.0

BF16, F32 = torch.bfloat16, torch.float32
CH_HEADER = 9 * 1024 * 4                 # bytes: 8 arrival counters 4 KB apart, then the error word and the arrival count of the last wait
SMALL = [s for s in R.CHAIN_SHAPES]
MASK_SHAPES = [(40, (48, 16)), (136, (256, 144, 16)), (264, (384, 32))]
X3_SHAPES = [(8, (16,)), (40, (48, 16)), (264, (384, 32)), (1000, (2048, 16))]
# (K0_a, widths_a, K0_b, widths_b): K0_a < K0_b across a k-split boundary, K0_a > K0_b with a second chain of one layer, equal depth at KSW 3 / 8
PAIR_SHAPES = [(40, (48, 16), 136, (48, 16)), (264, (384, 32), 40, (384,)), (1000, (512, 16), 392, (512, 16)), (8, (16,), 8, (16,))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hulc2_amd import kernels as kn

    kn.set_compute("bf16")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    K.report("tests/test_mlp_chain_kernel_gpu.py")
    print(f"[kcheck-time] tests/test_mlp_chain_kernel_gpu.py {time.time() - t0:.1f} s")


def _reference(build, *args, **kw):
    """the CPU references on at most 8 threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(8, n))
    try:
        return build(*args, **kw)
    finally:
        torch.set_num_threads(n)


def _gate(ok: bool, dev, what: str):
    """kn.mlp_chain_ok / mlp_chain2_ok: on a whole MI355X (256 compute units) none of the listed shapes may be turned away"""
    from hulc2_amd import kernels as kn

    if not ok:
        assert kn.device_cu_count(dev) < 256, f"{what}: kn.mlp_chain_ok turns a listed shape away on a 256-CU device"
        pytest.skip(f"{what}: the device has fewer than 256 compute units")


def _padded(dev, t64, dtype, lead_rows, pad_cols, col0):
    """t64 (rows, cols) stored as a slice of a wider, taller sentinel-filled buffer: row pitch cols + pad_cols, first column col0"""
    rows, cols = t64.shape
    buf = sentinel_full((rows + 2 * lead_rows) * (cols + pad_cols), dtype, dev).view(rows + 2 * lead_rows, cols + pad_cols)
    v = buf[lead_rows:lead_rows + rows, col0:col0 + cols]
    v.copy_(t64.to(dtype))
    assert torch.equal(v.double().cpu(), t64), "an operand is not exact in its storage type"
    return v


class _Chain:
    """device operands of one chain case, every pitch wider than the logical width"""

    def __init__(self, dev, case):
        self.case, self.M, self.K0, self.dev = case, case["M"], case["K0"], dev
        self.widths = R.chain_widths(case)
        self.x0 = _padded(dev, case["x0"], F32, 0, 12, 4)
        self.outs, self.layers = [], []
        for lay in case["layers"]:
            N = lay["W"].shape[0]
            W = _padded(dev, lay["W"], BF16, 1, 8, 0)
            W_lo = None if lay["W_lo"] is None else _padded(dev, lay["W_lo"], BF16, 1, 8, 0)
            bias = None if lay["bias"] is None else _padded(dev, lay["bias"].view(1, -1), F32, 0, 8, 4)[0]
            mask = None if lay["mask"] is None else _padded(dev, lay["mask"], F32, 0, 12, 8)
            out = Guarded(dev, self.M, N, ld=N + 4)
            self.outs.append(out)
            self.layers.append((W, bias, lay["relu"], mask, lay["mask_scale"], out.t) + ((W_lo,) if W_lo is not None else ()))

    def ok(self):
        from hulc2_amd import kernels as kn

        return kn.mlp_chain_ok(self.M, self.K0, self.widths, self.dev)

    def launch(self):
        from hulc2_amd import kernels as kn

        kn.mlp_chain(self.x0, self.layers, self.M)
        torch.cuda.synchronize()
        kn.check_faults(self.dev)

    def values(self):
        return [o.value() for o in self.outs]

    def guards(self, who):
        for l, o in enumerate(self.outs):
            o.assert_guards(f"{who} layer {l}")


def _launch2(a: _Chain, b: _Chain):
    from hulc2_amd import kernels as kn

    kn.mlp_chain2(a.x0, a.layers, a.M, b.x0, b.layers, b.M)
    torch.cuda.synchronize()
    kn.check_faults(a.dev)


def _exact(got, want64, what):
    got, want = got.detach().cpu().reshape(-1), want64.float().reshape(-1)
    assert torch.equal(want.double(), want64.reshape(-1)), f"{what}: the expected values are not fp32 numbers (a broken lattice)"
    bad = ~((got == want) | (got.isnan() & want.isnan()))
    if bad.any():
        i = int(bad.nonzero()[0])
        cols = want64.shape[-1]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference; first at row {i // cols}, "
                             f"column {i % cols}: kernel {got[i].item()!r}, reference {want[i].item()!r}")


def _check_exact(ch: _Chain, who):
    want = R.chain_free(ch.case)
    ch.guards(who)
    for l, (o, w) in enumerate(zip(ch.outs, want)):
        _exact(o.value(), w, f"{who} layer {l}")


def _run_exact(dev, case, who):
    ch = _Chain(dev, case)
    _gate(ch.ok(), dev, who)
    ch.launch()
    _check_exact(ch, who)
    first = ch.values()
    ch.launch()
    for l, (a, b) in enumerate(zip(first, ch.values())):
        same_bits(a, b, f"{who} layer {l}")
    return ch


def _run_pair_exact(dev, ca, cb, who):
    from hulc2_amd import kernels as kn

    a, b = _Chain(dev, ca), _Chain(dev, cb)
    _gate(kn.mlp_chain2_ok(a.M, a.K0, a.widths, b.M, b.K0, b.widths, dev), dev, who)
    _launch2(a, b)
    _check_exact(a, f"{who} chain a")
    _check_exact(b, f"{who} chain b")
    first = a.values() + b.values()
    _launch2(a, b)
    for l, (x, y) in enumerate(zip(first, a.values() + b.values())):
        same_bits(x, y, f"{who} output {l}")


# ------------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.CHAIN_M)
@pytest.mark.parametrize("K0,widths", SMALL)
def test_permutation_chain_is_bit_exact(dev, K0, widths, M):
    case = _reference(R.perm_chain, M, K0, widths, seed=M, amp=R.perm_amp(K0, widths))
    _run_exact(dev, case, f"permutation chain K0 {K0} widths {widths} M {M}")


@pytest.mark.parametrize("M", R.CHAIN_M)
@pytest.mark.parametrize("K0,widths", SMALL)
def test_dense_lattice_is_bit_exact(dev, K0, widths, M):
    kw = R.DEEP_KW if len(widths) > 3 else {}
    for name, variant in (("bias, relu on even layers", dict()), ("no bias, no relu", dict(bias=False, relu=False)), ("bias, relu", dict(relu=True))):
        case = _reference(R.dense_chain, M, K0, widths, seed=M + len(variant), **kw, **variant)
        _run_exact(dev, case, f"dense lattice ({name}) K0 {K0} widths {widths} M {M}")


def test_4096_lattices_are_bit_exact(dev):
    """one lattice case each: the 4096-wide layer occupies all 256 workgroups and feeds KSW = 32; the 4096-deep input runs KSW = 32 on the
    staged input"""
    K0, widths = R.CHAIN_SHAPES_4096[0]
    _run_exact(dev, _reference(R.perm_chain, 64, K0, widths, seed=64, amp=R.perm_amp(K0, widths)), f"permutation chain K0 {K0} widths {widths} M 64")
    K0, widths = R.CHAIN_SHAPES_4096[1]
    _run_exact(dev, _reference(R.dense_chain, 17, K0, widths, seed=17), f"dense lattice K0 {K0} widths {widths} M 17")


@pytest.mark.parametrize("M", R.CHAIN_M)
def test_mask_epilogue_is_bit_exact(dev, M):
    """the data-gradient path of functional.MLPFn: out = mask > 0 ? v * 1.25 : 0 with zeros, negatives and positives in the mask, relu also
    set (the mask wins), ld_mask > N"""
    for K0, widths in MASK_SHAPES:
        case = _reference(R.dense_chain, M, K0, widths, seed=M + 7, masks=True, **R.MASK_KW)
        assert all(lay["relu"] and (lay["mask"] == 0).any() and (lay["mask"] < 0).any() for lay in case["layers"] if lay["mask"].numel() >= 256)
        ch = _run_exact(dev, case, f"mask lattice K0 {K0} widths {widths} M {M}")
        assert any((v < 0).any() for v in ch.values()), "no negative value came through a mask: relu was not overridden anywhere"


@pytest.mark.parametrize("M", [1, 5, 16, 17, 32])
def test_split_operands_alone_are_bit_exact(dev, M):
    for K0, widths in X3_SHAPES:
        case = _reference(R.dense_chain, M, K0, widths, seed=M + 9, x3=True)
        assert (R.split(case["x0"])[1] != 0).any()
        _run_exact(dev, case, f"split-operand lattice K0 {K0} widths {widths} M {M}")


@pytest.mark.parametrize("Ma,Mb", R.CHAIN_PAIRS)
@pytest.mark.parametrize("K0a,wa,K0b,wb", PAIR_SHAPES)
def test_pair_is_bit_exact(dev, K0a, wa, K0b, wb, Ma, Mb):
    who = f"pair a (K0 {K0a}, {wa}, M {Ma}) b (K0 {K0b}, {wb}, M {Mb})"
    ca = _reference(R.dense_chain, Ma, K0a, wa, seed=Ma)
    cb = _reference(R.perm_chain, Mb, K0b, wb, seed=Mb, amp=R.perm_amp(K0b, wb))
    _run_pair_exact(dev, ca, cb, who + " dense / permutation")
    # the other way round, the second chain with a bias (skipping it for rows 32.. would show) and, where it has <= 2 layers, split operands
    ca = _reference(R.perm_chain, Ma, K0a, wa, seed=Ma + 1, amp=R.perm_amp(K0a, wa))
    cb = _reference(R.dense_chain, Mb, K0b, wb, seed=Mb + 1, relu=True)
    assert all(lay["bias"].abs().max() > 0 for lay in cb["layers"])
    _run_pair_exact(dev, ca, cb, who + " permutation / dense")
    if max(K0a, K0b) <= 2048:
        cb = _reference(R.dense_chain, Mb, K0b, wb, seed=Mb + 9, x3=True)
        _run_pair_exact(dev, ca, cb, who + " permutation / split operands")


# ------------------------------------------------------------------------------------------------
# random cases, teacher-forced per layer
# ------------------------------------------------------------------------------------------------
def _check_forced(ch: _Chain, kernel, who):
    got = ch.values()
    ref = _reference(R.chain_forced, ch.case, got)
    e32 = _reference(R.chain_forced, ch.case, got, R.chain_layer_emu32)
    ch.guards(who)
    for l, (g, a, b) in enumerate(zip(got, ref, e32)):
        compare_rows(kernel, f"{who} L{l}", g, a, b, MARGIN)


@pytest.mark.parametrize("K0,widths", SMALL + R.CHAIN_SHAPES_4096)
def test_random_chain_against_float64(dev, K0, widths):
    big = (K0, widths) in R.CHAIN_SHAPES_4096
    runs = [(64, False, False)] if big else [(17, False, False), (64, False, False), (5, True, False), (17, False, True), (1, False, False)]
    for M, masks, x3 in runs:
        if x3 and (K0, widths) not in X3_SHAPES:
            continue
        case = _reference(R.random_chain, M, K0, widths, seed=K0 + M, masks=masks, x3=x3)
        who = f"K0 {K0} N{widths[-1]}x{len(widths)} M{M}"
        ch = _Chain(dev, case)
        _gate(ch.ok(), dev, who)
        ch.launch()
        _check_forced(ch, "mlp_chain mask" if masks else "mlp_chain x3" if x3 else "mlp_chain", who)
        first = ch.values()
        ch.launch()
        for l, (a, b) in enumerate(zip(first, ch.values())):
            same_bits(a, b, f"{who} layer {l}")


@pytest.mark.parametrize("Ma,Mb", [(5, 17), (32, 32)])
def test_random_pair_against_float64(dev, Ma, Mb):
    from hulc2_amd import kernels as kn

    for K0a, wa, K0b, wb in PAIR_SHAPES[:3]:
        ca = _reference(R.random_chain, Ma, K0a, wa, seed=K0a + Ma)
        cb = _reference(R.random_chain, Mb, K0b, wb, seed=K0b + Mb, x3=K0b != 136)             # (plain / split operands / split operands)
        a, b = _Chain(dev, ca), _Chain(dev, cb)
        who = f"pair K0 {K0a}/{K0b} M {Ma}/{Mb}"
        _gate(kn.mlp_chain2_ok(a.M, a.K0, a.widths, b.M, b.K0, b.widths, dev), dev, who)
        _launch2(a, b)
        _check_forced(a, "mlp_chain2", who + " a")
        _check_forced(b, "mlp_chain2", who + " b")


@pytest.mark.parametrize("K0,widths", [s for s in SMALL if len(s[1]) > 1])
def test_last_layer_against_a_free_running_reference(dev, K0, widths):
    """hidden layers on the lattice (exact in fp32 and in bf16: no rounding can differ between kernel and reference), the last layer with
    continuous weights: the end-to-end path without teacher forcing, under the same bound"""
    kw = R.DEEP_KW if len(widths) > 3 else {}
    for M in (33, 64):
        case = _reference(R.dense_chain, M, K0, widths, seed=M + 11, last_random=True, **kw)
        ch = _Chain(dev, case)
        who = f"K0 {K0} N{widths[-1]}x{len(widths)} M{M}"
        _gate(ch.ok(), dev, who)
        ch.launch()
        ch.guards(who)
        ref, e32 = _reference(R.chain_free, case), _reference(R.chain_free, case, R.chain_layer_emu32)
        for l in range(len(widths) - 1):
            _exact(ch.outs[l].value(), ref[l], f"{who} hidden layer {l}")
        compare_rows("mlp_chain free", f"{who} last", ch.outs[-1].value(), ref[-1], e32[-1], MARGIN)


# ------------------------------------------------------------------------------------------------
# the workspace contract (C entry points, a workspace of the test's own)
# ------------------------------------------------------------------------------------------------
class _Workspace:
    """exactly `need` bytes inside guard bands of the bf16 NaN sentinel; the header zero, everything behind it zero or poisoned"""
    G = 64                                                            # int16 elements: 128 bytes, the workspace stays 16-byte aligned

    def __init__(self, dev, need: int, poison: bool):
        assert need % 2 == 0 and need > CH_HEADER
        self.need, self.n = need, need // 2
        self.buf = torch.full((self.G + self.n + self.G,), 0x7FC5, dtype=torch.int16, device=dev)
        self.ws = self.buf[self.G:self.G + self.n]
        self.ws[:CH_HEADER // 2] = 0
        if not poison:
            self.ws[CH_HEADER // 2:] = 0
        assert self.ws.data_ptr() % 16 == 0

    def check(self, who):
        g = self.G
        assert bool((self.buf[:g] == 0x7FC5).all()) and bool((self.buf[g + self.n:] == 0x7FC5).all()), \
            f"{who}: the kernel wrote outside the {self.need} bytes hulc_mlp_chain_workspace advertises"
        head = self.ws[:CH_HEADER // 2].view(torch.int32)
        bad = head.nonzero().reshape(-1).tolist()
        assert not bad, f"{who}: header words {bad[:8]} are not zero after the launch (counters at 1024-word steps, error word 8192, arrival count 8208)"


def _raw_launch(dev, chains, ws_ptr, descs=None):
    from hulc2_amd import kernels as kn, lib as L

    so = L.load()
    descs = descs or [kn._chain_desc(c.x0, c.layers, c.M, 1)[0] for c in chains]
    fw, st = kn.fault_word(dev).data_ptr(), kn._stream()
    if len(descs) == 1:
        L.check(so.hulc_mlp_chain(ctypes.byref(descs[0]), ws_ptr, fw, st), "hulc_mlp_chain")
    else:
        L.check(so.hulc_mlp_chain2(ctypes.byref(descs[0]), ctypes.byref(descs[1]), ws_ptr, fw, st), "hulc_mlp_chain2")


def _need(chains):
    from hulc2_amd import kernels as kn, lib as L

    return sum(L.load().hulc_mlp_chain_workspace(ctypes.byref(kn._chain_desc(c.x0, c.layers, c.M, 1)[0])) for c in chains)


def _own_workspace_run(dev, cases, who, poison):
    from hulc2_amd import kernels as kn

    chains = [_Chain(dev, c) for c in cases]
    w = _Workspace(dev, _need(chains), poison)
    _raw_launch(dev, chains, w.ws.data_ptr())
    torch.cuda.synchronize()
    kn.check_faults(dev)
    w.check(who)
    for i, ch in enumerate(chains):
        _check_exact(ch, f"{who} chain {i}")
    return [v for ch in chains for v in ch.values()]


WS_SINGLE = [(1, 8, (16,)), (5, 136, (256, 144, 16)), (17, 392, (512, 1024, 16)), (64, 24, (64, 16, 48, 32, 16, 64, 32, 16))]


@pytest.mark.parametrize("M,K0,widths", WS_SINGLE)
def test_workspace_bounds_poison_and_header(dev, M, K0, widths):
    """stale rows of the exchange regions (bf16 NaNs) may only reach rows that are never stored: bit-identical to the clean-workspace run;
    nothing outside the advertised bytes is written; the header is zero again"""
    kw = R.DEEP_KW if len(widths) > 3 else {}
    for name, case in (("dense", _reference(R.dense_chain, M, K0, widths, seed=M, **kw)),
                       ("permutation", _reference(R.perm_chain, M, K0, widths, seed=M, amp=R.perm_amp(K0, widths)))):
        who = f"own workspace {name} K0 {K0} widths {widths} M {M}"
        _gate(_Chain(dev, case).ok(), dev, who)
        clean = _own_workspace_run(dev, [case], who + " clean", False)
        dirty = _own_workspace_run(dev, [case], who + " poisoned", True)
        for l, (a, b) in enumerate(zip(clean, dirty)):
            same_bits(a, b, f"{who} layer {l}: a stale exchange row reached a live row")
    if M <= 32 and len(widths) <= 2:
        case = _reference(R.dense_chain, M, K0, widths, seed=M + 9, x3=True)
        _own_workspace_run(dev, [case], f"own workspace split operands K0 {K0} M {M}", True)


@pytest.mark.parametrize("x3", [False, True])
def test_pair_workspace_bounds_poison_and_header(dev, x3):
    for (Ma, Mb), (K0a, wa, K0b, wb) in (((5, 17), PAIR_SHAPES[0]), ((5, 17), PAIR_SHAPES[1]), ((32, 1), PAIR_SHAPES[3])):
        ca = _reference(R.dense_chain, Ma, K0a, wa, seed=Ma)
        cb = _reference(R.dense_chain, Mb, K0b, wb, seed=Mb + 9, x3=True) if x3 else _reference(R.perm_chain, Mb, K0b, wb, seed=Mb, amp=R.perm_amp(K0b, wb))
        who = f"own workspace pair K0 {K0a}/{K0b} M {Ma}/{Mb} x3 {x3}"
        clean = _own_workspace_run(dev, [ca, cb], who + " clean", False)
        dirty = _own_workspace_run(dev, [ca, cb], who + " poisoned", True)
        for l, (a, b) in enumerate(zip(clean, dirty)):
            same_bits(a, b, f"{who} output {l}: a stale exchange row reached a live row")


def test_two_chains_back_to_back_on_one_workspace(dev):
    """the last workgroup puts the header back: a different chain launched right behind on the same (poisoned) workspace comes out right,
    and so does the first one launched a third time"""
    from hulc2_amd import kernels as kn

    c1 = _reference(R.dense_chain, 17, 392, (512, 1024, 16), seed=3)
    c2 = _reference(R.perm_chain, 48, 40, (48, 16), seed=4)
    c3 = _reference(R.dense_chain, 5, 136, (256, 144, 16), seed=5, masks=True, **R.MASK_KW)
    chains = [_Chain(dev, c) for c in (c1, c2, c3)]
    w = _Workspace(dev, max(_need([c]) for c in chains), True)
    for ch in chains + chains[:1]:
        _raw_launch(dev, [ch], w.ws.data_ptr())
    torch.cuda.synchronize()
    kn.check_faults(dev)
    w.check("three chains back to back")
    for i, ch in enumerate(chains):
        _check_exact(ch, f"back to back chain {i}")


# ------------------------------------------------------------------------------------------------
# refusals: host-side checks that return before any launch
# ------------------------------------------------------------------------------------------------
MSG_SHAPE = "hulc_mlp_chain: N must be a multiple of 16, K a multiple of 8 and <= 4096, operands 16-byte aligned"
MSG_ROWS = "hulc_mlp_chain: 1 <= M <= 64 rows (32 per chain of a pair)"
MSG_KSW = "hulc_mlp_chain: K must round up to 128 x {1, 2, 3, 4, 8, 16, 32}"


def _plain(dev, M, K0, widths, x3=False, rows=None):
    """a valid chain of zeros (refusals never read it); rows: the rows of x0 and of the outputs when they differ from M"""
    rows = M if rows is None else rows
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    layers, k = [], K0
    for n in widths:
        layers.append(R._layer(z(n, k), z(n, k) if x3 else None, z(n)))
        k = n
    return _Chain(dev, dict(M=rows, K0=K0, x0=z(rows, K0), layers=layers, x3=x3))


def test_chain_refusals(dev):
    from hulc2_amd import kernels as kn

    def one(ch, msg, M=None, share=None):
        refused(lambda: kn.mlp_chain(ch.x0, ch.layers, ch.M if M is None else M, share), msg, *ch.outs)

    ch = _plain(dev, 64, 40, (48, 16))
    one(ch, MSG_ROWS, M=0)
    one(ch, MSG_ROWS, M=65)
    for K0, widths, msg in ((40, (24,), MSG_SHAPE), (8, (4112,), MSG_SHAPE), (4, (16,), MSG_SHAPE), (12, (16,), MSG_SHAPE), (520, (16,), MSG_KSW),
                            (40, (48, 640, 16), MSG_KSW)):
        one(_plain(dev, 8, K0, widths), msg)
    # 9 layers: the descriptor holds 8, the count says 9
    d = kn._chain_desc(ch.x0, ch.layers, ch.M, 1)[0]
    d.nl = 9
    w = _Workspace(dev, CH_HEADER + 4096, False)
    refused(lambda: _raw_launch(dev, None, w.ws.data_ptr(), [d]), "hulc_mlp_chain: 1..8 layers", *ch.outs)
    # misaligned operands, one at a time
    W, bias, relu, mask, ms, out = _plain(dev, 8, 40, (48,)).layers[0]
    x = torch.zeros(8, 44, device=dev)
    m = torch.zeros(8, 52, device=dev)
    o = Guarded(dev, 8, 48, ld=52)
    wflat, bflat = torch.zeros(48 * 40 + 8, device=dev, dtype=BF16), torch.zeros(56, device=dev)

    def lone(x0, layer, msg, *outs):
        refused(lambda: kn.mlp_chain(x0, [layer], 8), msg, *outs)

    lone(x[:, 1:41], (W, bias, relu, None, 1.0, o.t), "hulc_mlp_chain: input must be 16-byte aligned", o)
    lone(torch.zeros(8, 41, device=dev)[:, :40], (W, bias, relu, None, 1.0, o.t), "hulc_mlp_chain: input must be 16-byte aligned", o)      # ld_x0 % 4
    lone(x[:, :40], (wflat[4:4 + 48 * 40].view(48, 40), bias, relu, None, 1.0, o.t), MSG_SHAPE, o)
    lone(x[:, :40], (W, bflat[1:49], relu, None, 1.0, o.t), "hulc_mlp_chain: bias must be 16-byte aligned", o)
    lone(x[:, :40], (W, bias, relu, m[:, 1:49], 1.0, o.t), "hulc_mlp_chain: mask must be 16-byte aligned", o)
    o1 = Guarded(dev, 8, 48, ld=52, lead=1)
    lone(x[:, :40], (W, bias, relu, None, 1.0, o1.t), MSG_SHAPE, o1)
    # split operands
    c3 = _plain(dev, 8, 40, (48, 16), x3=True)
    some = [c3.layers[0], c3.layers[1][:6]]
    refused(lambda: kn.mlp_chain(c3.x0, some, 8), "hulc_mlp_chain: W_lo on every layer of the chain or on none", *c3.outs)
    c40 = _plain(dev, 40, 40, (48, 16), x3=True)
    one(c40, "hulc_mlp_chain: split operands take <= 32 rows")
    one(_plain(dev, 8, 4096, (16,), x3=True), "hulc_mlp_chain: split operands take K <= 2048")
    one(_plain(dev, 8, 40, (4096, 16), x3=True), "hulc_mlp_chain: split operands take K <= 2048")
    # the share of the device
    one(ch, "hulc_mlp_chain: coop_share is 0 (= 1), 1, 2 or 4", share=3)
    one(_plain(dev, 8, 40, (4096, 16)), "hulc_mlp_chain: the chain is wider than its share of the device (coop_share)", share=2)
    kn.check_faults(dev)


def test_pair_refusals(dev):
    from hulc2_amd import kernels as kn

    def two(a, b, msg, Ma=None, Mb=None):
        refused(lambda: kn.mlp_chain2(a.x0, a.layers, a.M if Ma is None else Ma, b.x0, b.layers, b.M if Mb is None else Mb), msg, *(a.outs + b.outs))

    a, b = _plain(dev, 33, 40, (48, 16)), _plain(dev, 33, 136, (48, 16))
    two(a, b, MSG_ROWS, Ma=33, Mb=8)
    two(a, b, MSG_ROWS, Ma=8, Mb=33)
    a, b = _plain(dev, 8, 40, (48, 16)), _plain(dev, 8, 136, (48, 16))
    two(_plain(dev, 8, 40, (48,)), b, "hulc_mlp_chain2: the first chain is the deeper one")
    two(a, _plain(dev, 8, 136, (64, 16)), "hulc_mlp_chain2: the chains have the same layer widths where both run")
    two(a, _plain(dev, 8, 520, (48, 16)), MSG_KSW)
    two(_plain(dev, 8, 40, (48, 16), x3=True), b, "hulc_mlp_chain2: split operands are the second chain's")
    # differing shares: the descriptors carry them
    da, db = kn._chain_desc(a.x0, a.layers, 8, 2)[0], kn._chain_desc(b.x0, b.layers, 8, 1)[0]
    w = _Workspace(dev, _need([a, b]), False)
    refused(lambda: _raw_launch(dev, None, w.ws.data_ptr(), [da, db]), "hulc_mlp_chain2: both chains carry the same coop_share", *(a.outs + b.outs))
    kn.check_faults(dev)
