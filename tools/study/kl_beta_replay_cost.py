"""what device-beta mode (Hulc2.set_kl_beta: the KL weight as a device scalar) costs per replayed step: ArenaTrainer.replay() on the benchmark
batch (B 32, S 32, bf16)
  base_a / base_b  a checkout of the PARENT commit with its library built (--baseline-tree), replay() as it was — the same leg twice: the
                   difference between the two is the box's run-to-run spread, the yardstick for the other legs
  value            this tree, no set_kl_beta: beta by value, the same launches as the parent
  device           this tree, ArenaTrainer.set_kl_beta(0.01) before capture() and a new value before every window: hulc_cat_kl_*_sched
                   inside the graph (one 4-byte load per thread), one 1-element fill per window outside it
Every leg is a fresh child process (one GPU process at a time); the legs alternate `--rounds` times so that drift of the box shows up as
spread inside a leg rather than as a difference between legs.  Per child: 2 eager steps, capture(), `--warmup` replays, then `--windows`
windows of `--steps` replays, each ended by a device synchronise; ms per step = host clock over the window.  Numbers from different boxes
differ by more than the legs do (README: +-2-3 %): compare inside one run of this script only.

    python tools/study/kl_beta_replay_cost.py --baseline-tree /path/to/parent/checkout [--rounds 3]"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parents[2]


def child(args):
    sys.path.insert(0, str(Path(args.tree).resolve()))
    import torch
    from hulc2_amd import kernels as kn, synthetic as syn
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config
    from hulc2_amd.trainer import ArenaTrainer
    import hulc2_amd
    assert Path(hulc2_amd.__file__).resolve().parents[1] == Path(args.tree).resolve(), hulc2_amd.__file__
    dev = torch.device("cuda:0")
    kn.set_compute("bf16")
    model = instantiate(default_model_config(gripper_control=True, dropout_p=0.1)).to(dev)
    syn.fill_state_dict_(model.state_dict(), 42)
    model.train()
    tr = ArenaTrainer(model, lr=2e-4, overlap=False)
    if args.device_beta:
        tr.set_kl_beta(0.01)
        assert model.kl_beta_on_device
    batch = syn.make_batch(42, 32, 32, device=dev)
    for db in batch.values():
        db.pop("plan_idx", None)
    for i in range(2):
        tr.step(batch, i)
    tr.capture(batch)
    for _ in range(args.warmup):
        tr.replay()
    ms = []
    for w in range(args.windows):
        if args.device_beta:
            tr.set_kl_beta(0.01 * (w + 1) / args.windows)          # (an epoch's worth of replays per value)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = tr.replay()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / args.steps * 1e3)
    kn.check_faults(dev)
    final = float(loss)
    assert final == final
    print("RESULT " + json.dumps({"ms": ms, "loss": final, "kl_beta": float(model.kl_beta)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree", help="checkout of the parent commit, library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--tree")
    ap.add_argument("--device-beta", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    legs = [("value", str(HERE), False), ("device", str(HERE), True)]
    if args.baseline_tree:
        legs = [("base_a", args.baseline_tree, False)] + legs + [("base_b", args.baseline_tree, False)]
    got = {name: [] for name, _, _ in legs}
    for r in range(args.rounds):
        for name, tree, dev_beta in legs:
            cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--tree", tree, "--steps", str(args.steps),
                   "--windows", str(args.windows), "--warmup", str(args.warmup)] + (["--device-beta"] if dev_beta else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not line:       # a failed leg ends the study: nothing more is started on the GPU
                sys.stderr.write(out.stderr[-4000:])
                raise SystemExit(f"leg {name} (round {r}) failed with exit status {out.returncode}")
            res = json.loads(line[0][7:])
            got[name] += res["ms"]
            print(f"round {r} {name:6s}: " + " ".join(f"{x:.4f}" for x in res["ms"]) + f" ms/step  (loss {res['loss']:.4f}, kl_beta {res['kl_beta']:.3e})",
                  flush=True)
    summary = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "windows": len(v)}
               for n, v in got.items()}
    if "base_a" in summary:
        summary["spread_base_a_vs_base_b_ms"] = round(abs(summary["base_a"]["median_ms"] - summary["base_b"]["median_ms"]), 4)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
