"""What gradient clipping costs on the benchmarked model's arena (ArenaTrainer(gradient_clip_val=...), hulc_grad_norm_clip).

  python tools/grad_clip_time.py [--rounds 30] [--skip-native]
      1. the norm pass alone (two launches between two events), COLD (1 GiB streamed through the caches in front of every round) and
         right BEHIND A WRITE of the gradient arena (what backward / the all-reduce leave: the arena is smaller than the Infinity Cache),
         with its rate over the 4 n bytes it reads — next to torch.sum over the same bytes under the same two conditions, the read row of
         tools/probe/hbm_stream.py at this byte count;
      2. optimizer_step() (the pass + the two derive launches, eager, as tools/optim_rules_time.py times it: `off` is that tool's `adam`
         line) of three Adam trainers — clipping off, by norm, by value — taking turns inside every round;
      3. the native captured step (capture / replay, 64 play-sequences of 32 steps, as bench.py's headline loop) with gradient_clip_val
         unset and set, medians over `rounds` blocks of 10 replays.
  HULC_LIB=<another build> python tools/grad_clip_time.py --skip-native
      the same for a library built with -DHULC_GRAD_NORM_NT=1 (stage 1 reading with the non-temporal hint): the A/B of the load policy.
Medians of event-timed regions after three warm-up rounds."""
import argparse
import statistics
import sys

sys.path.insert(0, '.')


def _timed(torch, fn, before=None):
    if before is not None:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def _model(torch, dev):
    from hulc2_amd import synthetic as syn
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config
    m = instantiate(default_model_config(gripper_control=True, dropout_p=0.1)).to(dev)
    syn.fill_state_dict_(m.state_dict(), 42)
    m.train()
    return m


def passes(rounds: int) -> None:
    import torch
    from hulc2_amd import kernels as kn, lib
    from hulc2_amd.trainer import ArenaTrainer

    dev = torch.device("cuda")
    kn.set_compute("bf16")
    print(f"library {lib.lib_path()}")
    tr = ArenaTrainer(_model(torch, dev), overlap=False)
    tr.flat_g.normal_()
    n, g = tr.total, tr.flat_g
    src = torch.randn(n, device=dev)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)      # 1 GiB: four times the Infinity Cache
    out = torch.zeros(2, device=dev)
    print(f"arena {n} elements ({n / 1e6:.2f} M, {4 * n / 1e6:.1f} MB of gradients)")
    cases = {"norm pass": lambda: kn.grad_norm_clip(g, n, 1.0, None, 1.0, out), "torch.sum ": lambda: torch.sum(g)}
    conditions = {"cold (1 GiB filled in front)": lambda: flush.fill_(1.0), "behind a write of the arena": lambda: g.copy_(src)}
    for cname, before in conditions.items():
        for name, fn in cases.items():
            ts = [_timed(torch, fn, before) for _ in range(rounds + 3)][3:]
            med = statistics.median(ts)
            print(f"{name} {cname:30s}: median {med:7.1f} us (min {min(ts):6.1f}, max {max(ts):6.1f}) of {len(ts)}  ->  {4 * n / med / 1e6:5.2f} TB/s over 4 n bytes")
    torch.cuda.synchronize()
    print(f"norm {float(out[0]):.6g} (float64 {float(g.double().norm()):.6g}), coefficient {float(out[1]):.6g}")

    # as tools/optim_rules_time.py: one trainer per case, taking turns inside every round (each pass runs behind the other trainers' passes,
    # 750 MB of arenas apiece, so no arena is resident in the Infinity Cache when its turn comes)
    tr.close()
    modes = {"off": {}, "norm": dict(gradient_clip_val=1.0), "value": dict(gradient_clip_val=1.0, gradient_clip_algorithm="value")}
    trainers = {}
    for mode, kw in modes.items():
        trainers[mode] = ArenaTrainer(_model(torch, dev), overlap=False, **kw)
        trainers[mode].flat_g.normal_()
    times = {k: [] for k in modes}
    for r in range(rounds + 3):
        for mode, t in trainers.items():
            kn.advance_step_state(dev, rng=False)
            us = _timed(torch, t.optimizer_step)
            if r >= 3:
                times[mode].append(us)
    kn.check_faults(dev)
    off = statistics.median(times["off"])
    for mode, ts in times.items():
        med = statistics.median(ts)
        print(f"optimizer_step() clipping {mode:5s} (eager, pass + derive launches): median {med:7.1f} us of {len(ts)} ({med - off:+6.1f} us against off)")
    for t in trainers.values():
        t.close()


def native(rounds: int, batch_size: int, seq_len: int) -> None:
    import torch
    from hulc2_amd import kernels as kn, synthetic as syn
    from hulc2_amd.trainer import ArenaTrainer

    dev = torch.device("cuda")
    kn.set_compute("bf16")
    res = {}
    for name, clip in (("unset", None), ("set (norm, 1.0)", 1.0), ("unset, again", None)):
        kn.reset_step_state(dev)
        tr = ArenaTrainer(_model(torch, dev), lr=2e-4, overlap=False, gradient_clip_val=clip)
        batch = syn.make_batch(42, batch_size, seq_len, device=dev)
        for db in batch.values():
            db.pop("plan_idx", None)
        for i in range(2):
            tr.step(batch, i)
        tr.capture(batch)
        ts = []
        for r in range(rounds + 3):
            t = _timed(torch, lambda: [tr.replay() for _ in range(10)]) / 10.0
            if r >= 3:
                ts.append(t)
        kn.check_faults(dev)
        res[name] = statistics.median(ts)
        extra = f", last gradient norm {tr.last_grad_norm():.4g}" if clip else ""
        print(f"captured step, gradient_clip_val {name:16s}: median {res[name] / 1e3:7.4f} ms/step over {len(ts)} blocks of 10 replays "
              f"(min {min(ts) / 1e3:.4f}, max {max(ts) / 1e3:.4f}){extra}")
        tr.close()
        del tr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32, help="play sequences per modality (bench.py's default: 64 per step)")
    ap.add_argument("--seq-len", type=int, default=32)
    ap.add_argument("--skip-native", action="store_true")
    ap.add_argument("--skip-passes", action="store_true")
    a = ap.parse_args()
    if not a.skip_passes:
        passes(a.rounds)
    if not a.skip_native:
        native(a.rounds, a.batch, a.seq_len)
