"""What the plan-recognition norms cost: (1) bench.py's headline configuration in the native captured loop (B = 32 per modality, S = 32, bf16,
ArenaTrainer capture / replay) with the posterior's switches at the yaml's values and with encoder_normalize and the
sinusoid table on, one trainer at a time in the order A B A B; (2) the two trunk launches alone (64 sequences x 32 positions, 2 layers,
dropout 0.1) without and with both LayerNorm stages, event-timed through kernels.start_timing.

    python tools/txl_norms_time.py [--rounds 20] [--steps 10]

Prints medians and one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_times(rounds, steps, batch_size, seq_len):
    import torch
    from hulc2_amd import kernels as kn, synthetic as syn
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config
    from hulc2_amd.trainer import ArenaTrainer

    dev = torch.device("cuda")
    on = dict(encoder_normalize=True, position_embedding=False)       # (the module still refuses positional_normalize)
    times = {"default": [], "norms_on": []}
    for name, kw in (("default", {}), ("norms_on", on)) * 2:
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
        print(f"{name:10s}: median {statistics.median(ts):.4f} ms per step over {len(ts)} rounds of {steps} steps (min {min(ts):.4f}, "
              f"max {max(ts):.4f}); loss {float(tr.static_loss):.4f}")
        times[name] += ts
        tr.close()
        del tr, m
        torch.cuda.empty_cache()
    return {n: round(statistics.median(ts), 4) for n, ts in times.items()}


def trunk_times(reps=50):
    import torch
    from hulc2_amd import functional as HF, kernels as kn

    dev = torch.device("cuda", 0)
    B, S, E = 64, 32, 128
    torch.manual_seed(3)
    layer = torch.nn.TransformerEncoderLayer(E, 8, dim_feedforward=2048, dropout=0.1)
    enc = torch.nn.TransformerEncoder(layer, num_layers=2, norm=None, enable_nested_tensor=False).to(dev)
    pos = torch.nn.Embedding(40, E).to(dev)
    lns = [torch.nn.LayerNorm(E).to(dev) for _ in range(2)]
    keys = {k: ("self_attn." + k if k.startswith(("in_proj", "out_proj")) else k) for k in HF._TXL_KEYS}
    layers = [{k: dict(m.named_parameters())[keys[k]] for k in HF._TXL_KEYS} for m in enc.layers]
    emb = torch.randn(B, S, E, device=dev, requires_grad=True)
    r = torch.randn(B, E, device=dev)
    ids = torch.arange(S, device=dev)
    out = {}
    for name, norms in (("plain", (None, None)), ("norms", tuple((ln.weight, ln.bias) for ln in lns))) * 2:
        def step():
            y = HF.transformer_trunk_pooled(emb, pos.weight, ids, layers, 8, 0.1, 1, *norms)
            (y * r).sum().backward()
        for _ in range(5):
            step()
        kn.start_timing()
        for _ in range(reps):
            step()
        rec = kn.stop_timing()
        for k, (n, ms, _, _) in rec.items():
            if "txl_block" in str(k[0]):
                out.setdefault(str(k[0]), []).append(round(ms / n * 1e3, 1))
    for k, v in sorted(out.items()):
        print(f"{k:24s} {v} us per launch (two passes of {reps})")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq-len", type=int, default=32)
    a = ap.parse_args()
    from hulc2_amd import kernels as kn

    kn.set_compute("bf16")
    trunk = trunk_times()
    steps = step_times(a.rounds, a.steps, a.batch, a.seq_len)
    print(json.dumps({"tool": "txl_norms_time", "batch_per_modality": a.batch, "seq_len": a.seq_len, "ms_per_step": steps, "trunk_us": trunk}))
