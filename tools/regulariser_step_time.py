"""What the encoder regularisers cost in the native captured loop: bench.py's headline configuration (B = 32 per modality, S = 32, bf16
compute, ArenaTrainer capture / replay) with the switches at their defaults and with dropout_vis_fc = 0.1, word_dropout_p = 0.1 and all
four l2 flags on, and with the decoder's policy_rnn_dropout_p = 0.1 alone, one trainer at a time in the order A B C A B C.

    python tools/regulariser_step_time.py [--rounds 20] [--steps 10]

Prints per configuration the median milliseconds per replayed step over `rounds` event-timed regions of `steps` steps, and one JSON line."""
import argparse
import json
import statistics
import sys

sys.path.insert(0, '.')


def main(rounds: int, steps: int, batch_size: int, seq_len: int) -> None:
    import torch
    from hulc2_amd import kernels as kn, synthetic as syn
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config
    from hulc2_amd.trainer import ArenaTrainer

    dev = torch.device("cuda")
    kn.set_compute("bf16")
    on = dict(dropout_vis_fc=0.1, word_dropout_p=0.1, l2_normalize_output=True, l2_normalize_goal_embeddings=True)
    times, loss = {"default": [], "regularisers_on": [], "rnn_dropout": []}, {}
    # A B C A B C, one live trainer at a time: each configuration sees the box twice
    for name, kw in (("default", {}), ("regularisers_on", on), ("rnn_dropout", dict(policy_rnn_dropout_p=0.1))) * 2:
        kn.reset_step_state(dev)
        m = instantiate(default_model_config(gripper_control=True, dropout_p=0.1, **kw)).to(dev)
        syn.fill_state_dict_(m.state_dict(), 42)
        m.train()
        tr = ArenaTrainer(m, lr=2e-4, overlap=False)
        batch = syn.make_batch(42, batch_size, seq_len, device=dev)
        for db in batch.values():
            db.pop("plan_idx", None)
        tr.capture(batch)
        ts = []
        for r in range(rounds // 2 + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                tr.replay()
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                ts.append(e0.elapsed_time(e1) / steps)
        kn.check_faults(dev)
        print(f"{name:16s}: median {statistics.median(ts):.4f} ms per step over {len(ts)} rounds of {steps} steps (min {min(ts):.4f}, "
              f"max {max(ts):.4f}); loss {float(tr.static_loss):.4f}")
        times[name] += ts
        tr.close()
        del tr, m
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "regulariser_step_time", "batch_per_modality": batch_size, "seq_len": seq_len,
                      "ms_per_step": {n: round(statistics.median(ts), 4) for n, ts in times.items()}}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq-len", type=int, default=32)
    a = ap.parse_args()
    main(a.rounds, a.steps, a.batch, a.seq_len)
