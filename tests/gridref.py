"""The padded-grid layout of the affordance kernels (include/hulc2_amd.h, "PADDED GRID"; csrc/gridconv.hip, affordance.hip, wgrad_taps.hip) for
tests/test_grid_kernels_gpu.py: test-owned grid fixtures inside sentinel allocations, the float64 references that are particular to the layout,
and replays of the launchers' host arithmetic (which kernel instance, how many workgroups / row groups / slices a shape gets).  Nothing here
needs a GPU: tests/test_gridref_cpu.py checks the layout against torch's conv2d and the replays against hand-computed plans.

A map (N, H, W, C) is R = N (H + 2)(W + 2) rows of C channels, pixel (n, y, x) = row n (H + 2)(W + 2) + (y + 1)(W + 2) + (x + 1), border rows
zero, and at least W + 3 zero rows before and behind."""
import torch

from tests.kcheck import GUARD, _SENTINEL, sentinel_full

BF = torch.bfloat16
TILE = 128                       # GC_BM of csrc/gridconv.hip: rows of a workgroup tile = rows of one statistics partial


def grid_R(N, H, W):
    return N * (H + 2) * (W + 2)


def interior_mask(N, H, W):
    """(R,) bool: the grid rows that are pixels"""
    m = torch.zeros(N, H + 2, W + 2, dtype=torch.bool)
    m[:, 1:-1, 1:-1] = True
    return m.reshape(-1)


def to_rows(x_nhwc):
    """(N, H, W, C) -> (R, C) grid rows with zero border rows"""
    N, H, W, C = x_nhwc.shape
    g = torch.zeros(N, H + 2, W + 2, C, dtype=x_nhwc.dtype)
    g[:, 1:-1, 1:-1] = x_nhwc
    return g.reshape(-1, C)


def from_rows(rows, N, H, W):
    """(R, C) grid rows -> the (N, H, W, C) pixels"""
    return rows.reshape(N, H + 2, W + 2, -1)[:, 1:-1, 1:-1]


def borders(rows, N, H, W):
    """the border rows of (R, C) grid rows"""
    return rows[~interior_mask(N, H, W).to(rows.device)]


def tap_offsets(W):
    """row offset of tap t = 3 (dy + 1) + (dx + 1)"""
    return [(t // 3 - 1) * (W + 2) + (t % 3 - 1) for t in range(9)]


def fwd_weights(w):
    """(Cout, Cin, 3, 3) -> [Cout][9 Cin], k = tap * Cin + ci (the forward operand of hulc_gridconv3x3)"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def dgrad_weights(w):
    """(Cout, Cin, 3, 3) -> [Cin][9 Cout] = (ci, kh, kw, co), taps NOT flipped: the data-gradient operand (flip_taps walks them backwards)"""
    return w.permute(1, 2, 3, 0).reshape(w.shape[1], -1).contiguous()


def conv_rows(xrows, wt, W, flip=False, guard=None):
    """the header's formula, literally: y[r][co] = sum_{t, ci} x[r + off_t][ci] wt[co][t Cin + ci] for EVERY grid row r (border rows included:
    the kernels force those to zero afterwards), rows outside the tensor read as zero.  flip: off_{8 - t}."""
    R, Cin = xrows.shape
    g = W + 3 if guard is None else guard
    z = torch.zeros(g, Cin, dtype=xrows.dtype)
    xp = torch.cat([z, xrows, z])
    y = torch.zeros(R, wt.shape[0], dtype=xrows.dtype)
    offs = tap_offsets(W)
    for t in range(9):
        o = offs[8 - t] if flip else offs[t]
        y += xp[g + o:g + o + R] @ wt[:, t * Cin:(t + 1) * Cin].t()
    return y


def taps_wgrad_rows(dzrows, xrows, W):
    """dW[co][ci][u] = sum_r dZ[r][co] X[r + off_u][ci] over the grid rows -> (Cout, Cin, 3, 3) (csrc/wgrad_taps.hip's header formula)"""
    R, Cin = xrows.shape
    g = W + 3
    z = torch.zeros(g, Cin, dtype=xrows.dtype)
    xp = torch.cat([z, xrows, z])
    return torch.stack([dzrows.t() @ xp[g + o:g + o + R] for o in tap_offsets(W)], -1).reshape(dzrows.shape[1], Cin, 3, 3)


def stats_partials(vrows, N, H, W):
    """(nb, 2, C): per 128-row tile the sums of v and v^2 over the tile's pixel rows (gridconv's `stats`)"""
    R, C = vrows.shape
    nb = (R + TILE - 1) // TILE
    v = torch.zeros(nb * TILE, C, dtype=vrows.dtype)
    v[:R] = vrows * interior_mask(N, H, W)[:, None].to(vrows.dtype)
    v = v.reshape(nb, TILE, C)
    return torch.stack([v.sum(1), (v * v).sum(1)], 1)


class GridBuf:
    """A test-owned bf16 grid tensor (N, H, W, C) with row pitch ld >= C inside a sentinel_full allocation:
         sentinel | exactly W + 3 zero rows | the R rows | (Rpad - R) + W + 3 zero rows | sentinel
    (Rpad = R rounded up to 32 with pad32 — the K of the weight-gradient products — else R); the padding columns of every row hold the sentinel.
    rows64 (R, C) given: an INPUT (the values, border rows as given — zero from to_rows()); None: an OUTPUT whose R rows hold the sentinel, so a
    kernel that skips a row (a border row it promises to zero) leaves a NaN.  `t` is the (R, C) view the kernel is handed (grid row 0; 16-byte
    aligned unless `lead`), `px0` the view at pixel (0, 0, 0) with `strides` = element strides (n, y, x) for the strided-map arguments."""

    def __init__(self, dev, N, H, W, C, ld=None, rows64=None, pad32=False, lead=0):
        self.N, self.H, self.W, self.C = N, H, W, C
        self.ld = ld = C if ld is None else ld
        assert ld >= C
        self.R = R = grid_R(N, H, W)
        self.Rpad = (R + 31) // 32 * 32 if pad32 else R
        self.pre, self.post = W + 3, (self.Rpad - R) + W + 3
        g0, n = GUARD + lead, (self.pre + R + self.post) * ld
        self.buf = sentinel_full(g0 + n + GUARD, BF, dev)
        allrows = self.buf[g0:g0 + n].view(-1, ld)
        allrows[:self.pre, :C] = 0
        allrows[self.pre + R:, :C] = 0
        self.full = allrows[self.pre:self.pre + R]
        self.t = self.full[:, :C]
        if rows64 is not None:
            assert tuple(rows64.shape) == (R, C)
            self.t.copy_(rows64.to(BF))
        self.px0 = self.full[W + 3:]
        self.strides = ((H + 2) * (W + 2) * ld, (W + 2) * ld, ld)
        assert lead or self.t.data_ptr() % 16 == 0
        self._snap = self.buf.clone()
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)
        inside[g0 + self.pre * ld:g0 + (self.pre + R) * ld].view(R, ld)[:, :C] = True
        self._outside = ~inside

    def assert_guards(self, what):
        it = _SENTINEL[BF][0]
        bad = int((self.buf.view(it)[self._outside] != self._snap.view(it)[self._outside]).sum())
        assert bad == 0, f"{what}: {bad} elements outside the {self.R} x {self.C} grid rows (zero guard rows, padding columns, sentinels) were overwritten"

    def assert_untouched(self, what):
        it = _SENTINEL[BF][0]
        assert torch.equal(self.buf.view(it), self._snap.view(it)), f"{what}: a refused call wrote to its output"

    def value(self):
        return self.t.detach().clone()

    def sentinel_rows(self):
        """(R,) bool: rows that still hold the sentinel in every channel (an output's rows the kernel did not write)"""
        it, bits = _SENTINEL[BF]
        return (self.t.view(it) == bits).all(1)


# ---- replays of the launchers' host arithmetic -------------------------------------------------------------------------------------------
def gridconv_path(Cin, Cout, R, cus, ldy=None, y_aligned=True):
    """csrc/gridconv.hip, gridconv_launch: the thin test (`ldy % 8 == 0 && ... Cin == 32 && (Cout == 32 || Cout == 64) ...`), GT_LAUNCH's
    `wgs = ((OCC * ncu + 7) / 8) * 8` with (Cin, NB, OCC) = (32, 1, 3) / (32, 2, 2) / (64, 1, 2), then `wide` and the GC_LAUNCH chain"""
    gx = (R + TILE - 1) // TILE
    ldy = Cout if ldy is None else ldy
    if ldy % 8 == 0 and y_aligned and ((Cin == 32 and Cout in (32, 64)) or (Cin == 64 and Cout == 32)):
        cin, nb, occ = (32, 1, 3) if Cout == 32 and Cin == 32 else ((32, 2, 2) if Cin == 32 else (64, 1, 2))
        return f"gridconv_thin<{cin},{nb}> wgs={(occ * cus + 7) // 8 * 8} tiles={gx}"
    wide = Cin % 64 == 0 and Cin >= 128
    if Cout % 128 == 0 and Cin % 128 == 0 and Cin >= 256 and gx * (Cout // 128) <= 320:
        inst, bn = "2,2,4", 128
    elif Cout % 128 == 0:
        inst, bn = ("2,2,2" if wide else "2,2,1"), 128
    elif Cout % 64 == 0:
        inst, bn = ("1,2,2" if wide else "1,2,1"), 64
    else:
        inst, bn = ("1,1,2" if wide else "1,1,1"), 32
    return f"gridconv<{inst}> grid={gx * (Cout // bn)} tiles={gx}"


def thin_trips(ntiles, wgs):
    """csrc/gridconv.hip, gridconv_thin_kernel: `per = (ntiles + 7) / 8` tiles per XCD walked by `nslots = gridDim.x >> 3` workgroups, tile
    += nslots: -> (per, nslots); a workgroup takes a second trip exactly when per > nslots"""
    return (ntiles + 7) // 8, wgs // 8


def bn_groups(nb, have_counters=True):
    """csrc/affordance.hip, hulc_grid_bn_finalize / hulc_grid_bn_relu_bwd: `while (G < 32 && nb / (G * 2) >= 64) G *= 2`"""
    G = 1
    if have_counters:
        while G < 32 and nb // (G * 2) >= 64:
            G *= 2
    return G


def plan_taps(M, N, K):
    """csrc/wgrad_taps.hip, plan_taps: -> dict(tiles, mode, kp, ksplit, kper)"""
    T = 64
    tm, tn = (M + T - 1) // T, (N + T - 1) // T
    mode = (1 if M == 32 else 0) | (2 if N == 32 else 0)
    kp = 1 if mode == 0 else (4 if mode == 3 else 2)
    nsteps = (K + T - 1) // T
    want = (nsteps + 64 * kp - 1) // (64 * kp)
    if nsteps <= 160 and tm * tn >= 32:
        want = 1
    want = max(1, min(want, 128))
    kper = (nsteps + want - 1) // want
    return dict(tiles=tm * tn, mode=mode, kp=kp, nsteps=nsteps, kper=kper, ksplit=(nsteps + kper - 1) // kper)


def head_wgrad_blocks(R, C):
    """csrc/affordance.hip, head_wgrad_blocks: -> (workgroups, rows of one pass of a workgroup)"""
    rpp = 256 // (C // 8)
    nb = (R + 8 * rpp - 1) // (8 * rpp)
    return min(max(nb, 1), 512), rpp


def upcat_bwd_npt(N, Cx, Hi, Wi, have_dg):
    """csrc/affordance.hip, hulc_grid_upcat_bwd: `if (!dg) while (N * (Cx / 64) * npt < 512 && npt * 64 < Hi * Wi) npt *= 2`"""
    npt = 1
    if not have_dg:
        while N * (Cx // 64) * npt < 512 and npt * 64 < Hi * Wi:
            npt *= 2
    return npt
