"""What gradient accumulation costs and saves in the native captured loop (ArenaTrainer(accumulate_grad_batches=k), hulc_grad_accumulate).

  python tools/grad_accum_time.py [--rounds 20] [--ks 1,2,4,8] [--windows 4]
      bench.py's headline configuration (64 play-sequences of 32 steps: B=32 per modality, bf16 compute, capture / replay), one trainer per
      k: two eager windows, capture() (two more), three warm-up rounds, then `rounds` rounds of `windows` whole windows between one event
      pair each.  Prints per k the median milliseconds per micro-batch and per window, and ONE JSON line with all of them at the end
      ({"ms_per_micro_batch": {k: ...}, "ms_per_window": {k: ...}}).  k = 1 is the plain captured step: bench.py's ms/step.
  python tools/grad_accum_time.py --kernel [--rounds 30]
      the accumulate pass alone on the benchmarked model's arena, its three modes taking turns with a 1 GiB fill in front of every launch
      (cold: inside a step a whole forward / backward lies between two passes), with the rate over the 8 / 12 / 12 bytes per element.
Run it alone on the GPU; every number is a median of event-timed regions."""
import argparse
import json
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
    return e0.elapsed_time(e1)


def _model(torch, dev):
    from hulc2_amd import synthetic as syn
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config
    m = instantiate(default_model_config(gripper_control=True, dropout_p=0.1)).to(dev)
    syn.fill_state_dict_(m.state_dict(), 42)
    m.train()
    return m


def kernel(rounds: int) -> None:
    import torch
    from hulc2_amd import kernels as kn
    from hulc2_amd.trainer import ArenaTrainer

    dev = torch.device("cuda")
    kn.set_compute("bf16")
    tr = ArenaTrainer(_model(torch, dev), overlap=False, accumulate_grad_batches=2)
    n, g, acc = tr.total, tr.flat_g, tr.flat_acc
    g.normal_()
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)      # 1 GiB: four times the Infinity Cache
    print(f"arena {n} elements ({n / 1e6:.2f} M)")
    times = {m: [] for m in ("store", "add", "finish")}
    for r in range(rounds + 3):
        for mode in times:
            ms = _timed(torch, lambda: kn.grad_accumulate(acc, g, n, mode, 0.5), lambda: flush.fill_(1.0))
            if r >= 3:
                times[mode].append(ms * 1e3)
    for mode, ts in times.items():
        med, per = statistics.median(ts), kn._ACC_MODES[mode][1]
        print(f"hulc_grad_accumulate {mode:6s} (cold): median {med:7.1f} us (min {min(ts):6.1f}, max {max(ts):6.1f}) of {len(ts)}  ->  "
              f"{per * n / med / 1e6:5.2f} TB/s over {per:.0f} n bytes")
    tr.close()


def windows(rounds: int, ks, per_round: int, batch_size: int, seq_len: int) -> None:
    import torch
    from hulc2_amd import kernels as kn, synthetic as syn
    from hulc2_amd.trainer import ArenaTrainer

    dev = torch.device("cuda")
    kn.set_compute("bf16")
    micro, window = {}, {}
    for k in ks:
        kn.reset_step_state(dev)
        tr = ArenaTrainer(_model(torch, dev), lr=2e-4, overlap=False, accumulate_grad_batches=k)
        batch = syn.make_batch(42, batch_size, seq_len, device=dev)
        for db in batch.values():
            db.pop("plan_idx", None)
        for i in range(2 * k):
            tr.step(batch, i)
        tr.capture(batch)
        ts = []
        for r in range(rounds + 3):
            ms = _timed(torch, lambda: [tr.replay() for _ in range(per_round * k)]) / per_round
            if r >= 3:
                ts.append(ms)
        kn.check_faults(dev)
        assert tr.micro_batch == 0
        window[k] = statistics.median(ts)
        micro[k] = window[k] / k
        print(f"accumulate_grad_batches {k}: median {micro[k]:7.4f} ms per micro-batch, {window[k]:8.4f} ms per window over {len(ts)} rounds of "
              f"{per_round} windows (window min {min(ts):.4f}, max {max(ts):.4f}); loss {float(tr.static_loss):.4f}")
        tr.close()
        del tr
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "grad_accum_time", "batch_per_modality": batch_size, "seq_len": seq_len,
                      "ms_per_micro_batch": {str(k): round(v, 4) for k, v in micro.items()},
                      "ms_per_window": {str(k): round(v, 4) for k, v in window.items()}}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--windows", type=int, default=4, help="whole windows between one event pair")
    ap.add_argument("--batch", type=int, default=32, help="play sequences per modality (bench.py's default: 64 per step)")
    ap.add_argument("--seq-len", type=int, default=32)
    ap.add_argument("--kernel", action="store_true", help="time the accumulate pass alone instead of the captured loop")
    a = ap.parse_args()
    if a.kernel:
        kernel(a.rounds)
    else:
        windows(a.rounds, [int(k) for k in a.ks.split(",")], a.windows, a.batch, a.seq_len)
