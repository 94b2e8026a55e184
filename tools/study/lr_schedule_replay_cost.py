"""what an attached learning-rate schedule costs per replayed step: ArenaTrainer.replay() on the benchmark batch (B 32, S 32, bf16)
  base   a checkout of the PARENT commit with its library built (--baseline-tree), replay() as it was
  plain  this tree, no schedule: the same launches as `base` (hulc_adam_step_lo, no fill)
  sched  this tree, set_lr_schedule(linear warm-up): one 1-element fill in front of the optimizer graph, hulc_adam_step_sched inside it
Every leg is a fresh child process (one GPU process at a time); the legs alternate `--rounds` times so that drift of the box shows up as
spread inside a leg rather than as a difference between legs.  Per child: 2 eager steps, capture(), `--warmup` replays, then `--windows`
windows of `--steps` replays, each ended by a device synchronise; ms per step = host clock over the window.  Numbers from different boxes
differ by more than the legs do (README: +-2-3 %): compare inside one run of this script only.

    python tools/study/lr_schedule_replay_cost.py --baseline-tree /path/to/parent/checkout [--rounds 3]"""
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
    if args.schedule:
        from hulc2_amd.optim import lr_lambda_from_config
        tr.set_lr_schedule(lr_lambda_from_config({"_target_": "transformers.get_linear_schedule_with_warmup",
                                                  "num_training_steps": 100000, "num_warmup_steps": 1000}))
    batch = syn.make_batch(42, 32, 32, device=dev)
    for db in batch.values():
        db.pop("plan_idx", None)
    for i in range(2):
        tr.step(batch, i)
    tr.capture(batch)
    for _ in range(args.warmup):
        tr.replay()
    ms = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = tr.replay()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / args.steps * 1e3)
    kn.check_faults(dev)
    final = float(loss)
    assert final == final
    print("RESULT " + json.dumps({"ms": ms, "loss": final, "lr": float(tr.lr)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree", help="checkout of the parent commit, library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--tree")
    ap.add_argument("--schedule", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    legs = [("plain", str(HERE), False), ("sched", str(HERE), True)]
    if args.baseline_tree:
        legs.insert(0, ("base", args.baseline_tree, False))
    got = {name: [] for name, _, _ in legs}
    for r in range(args.rounds):
        for name, tree, sched in legs:
            cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--tree", tree, "--steps", str(args.steps),
                   "--windows", str(args.windows), "--warmup", str(args.warmup)] + (["--schedule"] if sched else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not line:       # a failed leg ends the study: nothing more is started on the GPU
                sys.stderr.write(out.stderr[-4000:])
                raise SystemExit(f"leg {name} (round {r}) failed with exit status {out.returncode}")
            res = json.loads(line[0][7:])
            got[name] += res["ms"]
            print(f"round {r} {name:5s}: " + " ".join(f"{x:.4f}" for x in res["ms"]) + f" ms/step  (loss {res['loss']:.4f}, lr {res['lr']:.3e})", flush=True)
    summary = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "windows": len(v)}
               for n, v in got.items()}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
