import os, sys, torch
sys.path.insert(0, '.')
if int(os.environ.get("HULC_RNN_DBG") or 0) & 8:      # phase stamps: the instance exists in the -DHULC_PROBES build only
    sys.path.insert(0, 'tools/probe')
    import _build
    _build.use_probe_library()
from hulc2_amd import kernels as kn
dev = torch.device('cuda')
S, H = 32, 2048
P_DROP, SITE = 0.1, 0x5EED7001                        # the sweep with inter-layer dropout beside the plain one (hulc_rnn_wavefront_drop)
g = torch.Generator().manual_seed(0)
w = [((torch.rand(H, H, generator=g) * 2 - 1) * H ** -0.5).to(dev).to(torch.bfloat16) for _ in range(3)]
b = [torch.zeros(H, device=dev) for _ in range(3)]


def timed(f):
    for _ in range(2): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 5 * 1e3


for B in (64, 48, 32, 16, 8):
    pre0 = torch.randn(S, B, H, generator=g).to(dev)
    for tr in (False, True):
        zbuf = torch.zeros(S + 2, B, 2 * H, device=dev)
        kw = dict(add1=pre0, add1_step=B * H, ld_add1=H, bias1=(b[0], None), bias2=(b[1], b[2]), relu=True)
        us = timed(lambda: kn.rnn_wavefront(zbuf[0], B * 2 * H, S, B, H, w[0], w[1], w[2], tr, **kw))
        print(f"rnn_wavefront B={B} transposed={tr}: {us:.1f} us per pass, {us / (S + 1):.2f} us per wave step")
        # the forward sweep masks the product's inputs (keep bits from a launch in front, counted here), the transposed one its outputs
        mode, t0, t_dir = (kn.RNN_DROP_N, S, -1) if tr else (kn.RNN_DROP_K, -1, 1)
        usd = timed(lambda: kn.rnn_wavefront_drop(zbuf[0], B * 2 * H, S, B, H, w[0], w[1], w[2], tr, P_DROP, SITE, mode, t0, t_dir, **kw))
        print(f"rnn_wavefront_drop B={B} transposed={tr} p={P_DROP} mode={'N' if tr else 'K'}: {usd:.1f} us per pass ({usd / us:.3f} x plain)")
kn.check_faults(dev)
