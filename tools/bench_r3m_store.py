"""The real-world config (R3M static camera, 150 x 200) trained on episode-store windows: the static camera read in place, against what a user
had to do before VisionR3M took uint8 frames — gather the windows' frames with torch and convert them to fp32 NCHW every step.

Both feeds run the same captured step (ArenaTrainer graph mode, B windows per modality, S steps) on the same window draws; the `fp32` feed
adds, in front of every replay, `store[index]` + a converting copy into a fixed (B, S, 3, H, W) fp32 buffer per modality.  The feeds are
timed alternately, `--rounds` times, so the spread is visible.  The staging kernel's own time (hulc_r3m_stage_u8 on one modality's B * S
frames, packed bf16 output) is taken with device events next to the pieces it replaces (the torch gather + convert, hulc_r3m_normalize_packed).
No threshold: prints one JSON line.

    python tools/bench_r3m_store.py [--batch 32] [--seq-len 32] [--steps 30] [--warmup 5] [--rounds 2] [--store-frames 4096]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from hulc2_amd import kernels as kn, synthetic as syn  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import real_world_model_config  # noqa: E402
from hulc2_amd.datasets import DeviceEpisodeStore  # noqa: E402
from hulc2_amd.models.perceptual_encoders import vision_r3m as VR  # noqa: E402
from hulc2_amd.trainer import ArenaTrainer  # noqa: E402

H, W = 150, 200


def make_stores(dev, n, S):
    g = torch.Generator().manual_seed(99)
    rgb = {"rgb_static": torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).to(dev),
           "rgb_gripper": torch.randint(0, 256, (n, 84, 84, 3), generator=g, dtype=torch.uint8).to(dev)}
    act = torch.rand(n, 7, generator=g) * 2 - 1
    act[:, 6] = torch.where(act[:, 6] > 0, 1.0, -1.0)
    obs = torch.randn(n, 15, generator=g)
    eps = [(a, min(a + 511, n - 1)) for a in range(0, n, 512)]
    kw = dict(device=dev, aug_pad={"rgb_static": 0})                 # real_world_r3m.yaml: no RandomShiftsAug on the static camera
    lo = min(20, S)
    vis = DeviceEpisodeStore(rgb, act, obs, eps, lo, S, seed=0, **kw)
    spans = [(a + 64 * j, a + 64 * j + 63) for a, b in eps for j in range(0, (b - a + 1) // 64, 2)]
    lang_data = {"language": {"ann": [""] * len(spans), "task": [""] * len(spans),
                              "emb": (torch.randn(len(spans), 1, 384, generator=g) * 0.05).numpy()}, "info": {"indx": spans}}
    lang = DeviceEpisodeStore.from_language_annotations(vis.rgb, act, obs, lang_data, min_window_size=lo, max_window_size=S, seed=0, **kw)
    return {"vis": vis, "lang": lang}


class Feed:
    """one model + trainer + stores; draw() refreshes the batch in place (and, fp32 feed, materialises the static camera's frames)"""

    def __init__(self, dev, args, fp32: bool):
        self.fp32, self.args = fp32, args
        model = instantiate(real_world_model_config(dropout_p=0.1)).to(dev)
        syn.fill_state_dict_(model.state_dict(), 42)
        model.train()
        self.trainer = ArenaTrainer(model, lr=2e-4, overlap=False)
        self.stores = make_stores(dev, args.store_frames, args.seq_len)
        self.sampler = np.random.RandomState(1000)
        self.frames = {mod: torch.empty(args.batch, args.seq_len, 3, H, W, device=dev) for mod in self.stores} if fp32 else None
        self.batch = {}
        self.draw()
        for i in range(2):
            self.trainer.step(self.batch, i)
        self.trainer.capture(self.batch)

    def draw(self):
        for mod, st in self.stores.items():
            fresh = st.batch(self.sampler.randint(0, len(st), self.args.batch))
            fresh.pop("window_sizes")
            if self.fp32:
                rgb = dict(fresh["rgb_obs"])
                ix = rgb.pop("rgb_static_index")
                gathered = st.rgb["rgb_static"][ix.reshape(-1).long()]                       # (B * S, H, W, 3) uint8
                self.frames[mod].view(-1, 3, H, W).copy_(gathered.permute(0, 3, 1, 2))       # -> fp32 NCHW, [0, 255]
                rgb["rgb_static"] = self.frames[mod]
                fresh["rgb_obs"] = rgb
            self.batch[mod] = fresh

    def run(self, steps):
        for _ in range(steps):
            self.draw()
            loss = self.trainer.replay()
        return loss

    def timed(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = self.run(steps)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps, float(loss)


def event_ms(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_times(dev, feed, n):
    st = feed.stores["vis"]
    store, ix = st.rgb["rgb_static"], st.batch(np.arange(feed.args.batch))["rgb_obs"]["rgb_static_index"].reshape(-1)
    xp = torch.empty(n, H + 6, kn.r3m_packed_width(W), 4, dtype=torch.bfloat16, device=dev)
    lut = VR._byte_lut("real_world_r3m", VR.IMAGENET_MEAN, VR.IMAGENET_STD, torch.bfloat16, dev)
    x = torch.empty(n, 3, H, W, device=dev)
    out = {"r3m_stage_u8_ms": event_ms(lambda: kn.r3m_stage_u8(store, xp, lut, ix)),
           "torch_gather_convert_ms": event_ms(lambda: x.copy_(store[ix.long()].permute(0, 3, 1, 2))),
           "r3m_normalize_packed_ms": event_ms(lambda: kn.r3m_normalize_packed(x, xp, VR.IMAGENET_MEAN, VR.IMAGENET_STD))}
    return {k: round(v, 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32, help="windows per modality")
    ap.add_argument("--seq-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--store-frames", type=int, default=4096, help="frames in the synthetic store (90 KB + 21 KB each)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_r3m_store.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    kn.set_compute("bf16")
    feeds = {"store": Feed(dev, args, fp32=False), "fp32": Feed(dev, args, fp32=True)}
    for f in feeds.values():
        f.run(args.warmup)
    ms = {k: [] for k in feeds}
    for _ in range(args.rounds):
        for k, f in feeds.items():
            t, loss = f.timed(args.steps)
            if loss != loss:
                raise SystemExit(f"[bench_r3m_store] the loss of the {k} feed is NaN")
            ms[k].append(round(t, 4))
    kn.check_faults(dev)
    n = args.batch * args.seq_len
    print(json.dumps({"config": "real-world (R3M static 150x200), bf16, ArenaTrainer graphs, new store windows every step",
                      "batch_per_modality": args.batch, "seq_len": args.seq_len, "steps": args.steps, "rounds": args.rounds,
                      "ms_per_step_in_place": ms["store"], "ms_per_step_torch_gather_to_fp32": ms["fp32"],
                      "one_modality_frames": n, **kernel_times(dev, feeds["store"], n)}))


if __name__ == "__main__":
    main()
