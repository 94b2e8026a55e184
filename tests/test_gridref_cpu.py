"""tests/gridref.py without a GPU: the grid layout and the literal row formulas against torch's conv2d in float64, the fixture's layout, and the
replays of the launchers' host arithmetic at plans worked out by hand from the sources."""
import torch
import torch.nn.functional as F

from tests import gridref as G
from tests.kcheck import _SENTINEL


def _ints(g, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def test_row_formula_is_conv2d_forward_data_and_weight_gradient():
    g = torch.Generator().manual_seed(3)
    N, H, W, Cin, Cout = 2, 5, 4, 6, 7
    x = _ints(g, N, Cin, H, W).requires_grad_(True)
    w = (_ints(g, Cout, Cin, 3, 3) / 8).requires_grad_(True)
    dy = _ints(g, N, Cout, H, W)
    y = F.conv2d(x, w, padding=1)
    y.backward(dy)
    m = G.interior_mask(N, H, W)
    xr, dyr = G.to_rows(x.detach().permute(0, 2, 3, 1)), G.to_rows(dy.permute(0, 2, 3, 1))
    assert xr.shape == (G.grid_R(N, H, W), Cin) and not G.borders(xr, N, H, W).any()
    assert torch.equal(G.from_rows(xr, N, H, W), x.detach().permute(0, 2, 3, 1))
    yr = G.conv_rows(xr, G.fwd_weights(w.detach()), W) * m[:, None]
    assert torch.equal(G.from_rows(yr, N, H, W), y.detach().permute(0, 2, 3, 1))
    dxr = G.conv_rows(dyr, G.dgrad_weights(w.detach()), W, flip=True) * m[:, None]
    assert torch.equal(G.from_rows(dxr, N, H, W), x.grad.permute(0, 2, 3, 1))
    assert not torch.equal(G.conv_rows(dyr, G.dgrad_weights(w.detach()), W) * m[:, None], dxr)        # the asymmetric filter tells the flip
    assert torch.equal(G.taps_wgrad_rows(dyr, xr, W), w.grad)
    # the promised guard is exactly what the formula needs: W + 3 rows on either side, and one fewer is too few
    assert torch.equal(G.conv_rows(xr, G.fwd_weights(w.detach()), W, guard=W + 3), G.conv_rows(xr, G.fwd_weights(w.detach()), W, guard=W + 40))
    assert max(abs(o) for o in G.tap_offsets(W)) == W + 3


def test_stats_partials_follow_the_row_tiles():
    N, H, W, C = 3, 9, 9, 2
    v = torch.arange(G.grid_R(N, H, W) * C, dtype=torch.float64).reshape(-1, C)
    st = G.stats_partials(v, N, H, W)
    m = G.interior_mask(N, H, W)
    assert st.shape == (3, 2, C)                       # 363 rows: tiles of 128, 128, 107
    for b in range(3):
        rows = v[b * 128:(b + 1) * 128][m[b * 128:(b + 1) * 128]]
        assert torch.equal(st[b, 0], rows.sum(0)) and torch.equal(st[b, 1], (rows * rows).sum(0))
    assert torch.equal(st[:, 0].sum(0), v[m].sum(0))


def test_fixture_layout():
    dev = torch.device("cpu")
    it, bits = _SENTINEL[torch.bfloat16]
    N, H, W, C, ld = 2, 3, 5, 8, 16
    rows = G.to_rows(torch.ones(N, H, W, C, dtype=torch.float64))
    for pad32, rows64 in ((False, rows), (True, None)):
        gb = G.GridBuf(dev, N, H, W, C, ld=ld, rows64=rows64, pad32=pad32)
        R = N * 5 * 7
        assert gb.R == R == 70 and gb.pre == W + 3 and gb.post == (26 if pad32 else 0) + W + 3 and gb.Rpad == (96 if pad32 else 70)
        raw = gb.buf.view(it)
        assert (raw[:64] == bits).all() and (raw[-64:] == bits).all()
        body = raw[64:-64].view(-1, ld)
        assert body.shape[0] == gb.pre + R + gb.post
        assert (body[:, C:] == bits).all()                                  # padding columns
        assert (body[:gb.pre, :C] == 0).all() and (body[gb.pre + R:, :C] == 0).all()
        if rows64 is None:
            assert (body[gb.pre:gb.pre + R, :C] == bits).all() and gb.sentinel_rows().all()
        else:
            assert torch.equal(gb.value().double(), rows) and not gb.sentinel_rows().any()
        assert gb.t.data_ptr() % 16 == 0 and gb.px0.data_ptr() - gb.t.data_ptr() == (W + 3) * ld * 2
        assert gb.strides == (35 * ld, 7 * ld, ld)
        gb.assert_guards("fresh")
        gb.t[0, 0] = 1.0
        gb.assert_guards("a write inside the rows")
        gb.full[0, C] = 1.0
        try:
            gb.assert_guards("padding column")
        except AssertionError:
            pass
        else:
            raise AssertionError("a write to a padding column went unnoticed")
    gb = G.GridBuf(dev, 1, 2, 2, 8, rows64=None)
    gb.buf[64 + 8 * 2] = 1.0                                                # a zero guard row
    try:
        gb.assert_guards("guard row")
    except AssertionError:
        pass
    else:
        raise AssertionError("a write to a zero guard row went unnoticed")
    assert G.GridBuf(dev, 1, 2, 2, 8, lead=1).t.data_ptr() % 16 == 2


def test_launcher_replays():
    # gridconv_launch's dispatch on 256 CUs
    P = lambda ci, co, R, **k: G.gridconv_path(ci, co, R, 256, **k).split()[0]
    assert G.gridconv_path(32, 32, 234, 256) == "gridconv_thin<32,1> wgs=768 tiles=2"
    assert G.gridconv_path(32, 64, 234, 256) == "gridconv_thin<32,2> wgs=512 tiles=2"
    assert G.gridconv_path(64, 32, 112, 256) == "gridconv_thin<64,1> wgs=512 tiles=1"
    assert G.gridconv_path(32, 32, 234, 256, ldy=36) == "gridconv<1,1,1> grid=2 tiles=2"
    assert P(32, 64, 234, ldy=68) == "gridconv<1,2,1>" and P(64, 32, 100, y_aligned=False) == "gridconv<1,1,1>"
    assert P(256, 128, 56) == "gridconv<2,2,4>" and P(128, 128, 56) == "gridconv<2,2,2>" and P(96, 128, 56) == "gridconv<2,2,1>"
    assert P(256, 128, 128 * 321) == "gridconv<2,2,2>"                      # more than 320 workgroups: back to 64-channel k-steps
    assert P(128, 64, 56) == "gridconv<1,2,2>" and P(64, 64, 56) == "gridconv<1,2,1>" and P(192, 192, 56) == "gridconv<1,2,2>"
    assert P(128, 32, 56) == "gridconv<1,1,2>" and P(128, 96, 56) == "gridconv<1,1,2>" and P(96, 96, 56) == "gridconv<1,1,1>"
    assert G.gridconv_path(128, 96, 300, 256) == "gridconv<1,1,2> grid=9 tiles=3"
    # the persistent walk: 545 tiles never give the 96 slots of the 32 -> 32 instance a second trip, 781 do
    assert G.thin_trips(545, 768) == (69, 96) and G.thin_trips(545, 512) == (69, 64) and G.thin_trips(781, 768) == (98, 96)
    assert G.grid_R(4, 130, 130) == 545 * 128 - 64 and (G.grid_R(4, 156, 156) + 127) // 128 == 781
    # last-arriver row groups
    assert [G.bn_groups(n) for n in (5, 127, 128, 255, 256, 2047, 2048, 100000)] == [1, 1, 2, 2, 4, 16, 32, 32] and G.bn_groups(4096, False) == 1
    assert (G.grid_R(2, 126, 126) + 255) // 256 == 128
    # nine-tap plans
    assert G.plan_taps(64, 64, 96)["ksplit"] == 1 and [G.plan_taps(*mn, 96)["kp"] for mn in ((64, 64), (32, 64), (64, 32), (32, 32))] == [1, 2, 2, 4]
    K2 = (G.grid_R(2, 46, 46) + 31) // 32 * 32
    assert (K2, G.plan_taps(64, 64, K2)["ksplit"], G.plan_taps(64, 64, K2)["kper"]) == (4608, 2, 36)
    K17 = (G.grid_R(1, 255, 255) + 31) // 32 * 32
    assert (K17, G.plan_taps(64, 64, K17)["nsteps"], G.plan_taps(64, 64, K17)["ksplit"]) == (66080, 1033, 17)
    assert G.plan_taps(128, 192, 608) == dict(tiles=6, mode=0, kp=1, nsteps=10, kper=10, ksplit=1)
    # the head's weight gradient and the up-sampling backward
    assert G.head_wgrad_blocks(336, 64) == (2, 32) and G.head_wgrad_blocks(56, 8) == (1, 256) and G.head_wgrad_blocks(10 ** 7, 32) == (512, 64)
    assert G.upcat_bwd_npt(2, 64, 9, 9, False) == 2 and G.upcat_bwd_npt(2, 64, 9, 9, True) == 1 and G.upcat_bwd_npt(2, 64, 8, 8, False) == 1


def test_lattice_stays_exact_up_to_256_channels():
    """the precondition the GPU cases assert, at the largest lattice case: Cin 256 at 2 x 14 x 14 — every tile's sum of (8 y)^2 below 2^24"""
    g = torch.Generator().manual_seed(11)
    N, H, W, Cin, Cout = 2, 14, 14, 256, 32
    x, w = _ints(g, N, Cin, H, W), _ints(g, Cout, Cin, 3, 3) / 8
    y = G.to_rows(F.conv2d(x, w, padding=1).permute(0, 2, 3, 1))
    st = G.stats_partials(y * 8, N, H, W)
    assert st[:, 1].max().item() < 2 ** 24 and st[:, 1].sum(0).max().item() < 2 ** 24
