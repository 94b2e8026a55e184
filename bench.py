#!/usr/bin/env python3
"""Headline benchmark: play-sequences/sec/node of the HULC++ low-level policy training step on MI355X.

  python bench.py --gpus N --steps K --warmup W          (N > 1: launched by torch.distributed.run, one rank / GPU)
  python bench.py --gpus N --steps K --warmup W --full   (+ everything beyond the headline, listed below)
  python bench.py ... --dump-outputs DIR                 (+ what the last timed step computed, as DIR/<name>.npy)

A "step" = one full optimizer step of `Hulc2.training_step` (forward + backward + gradient all-reduce + Adam) over
one device-resident synthetic CALVIN-shaped batch: 2 modalities x 32 play sequences x 32 timesteps, 200x200 static +
84x84 gripper RGB, random (B,384) language embeddings (BASELINE.json configs[1]/[2]).  Weak scaling:
each rank processes its own 64 sequences per step.

A plain run sets up, warms up, times the K steps and prints ONE JSON line (rank 0) with the contract fields.  --full adds
  roofline     — the dominant kernel's algorithmic FLOP/s from HIP events recorded live on the launch stream (3 more eager steps)
  roofline_txl — the transformer trunk's launches inside the step and alone at 256 / 1024 sequences
  secondary*   — the step in the other arithmetic modes and the Lightning-style loop (--no-secondary skips them)
  cpu_baseline — the CPU oracle (fp32 torch restatement, kind "port") timed on this box's host cores on a bounded sample
                 (--no-cpu-baseline skips it)
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

SEQ_FLOP_TRAIN = 14.13e9        # 3 x 4.710 GFLOP forward per play sequence
PEAK_BF16 = 2.5e15              # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32 = 157.3e12
PEAK_HBM = 8.0e12               # HBM3E bytes/s (MI355X_MICROARCH.md)


# device kernel behind a timed (entry point, shape): kernel name prefix in the committed --pmc passes.  One kernel instance serves the
# static and the gripper camera (told apart in the passes by LDS size / grid): "max" = its launches with the larger traffic (static frames)
# (prefixes of the kernel names in profiles/*_pmc_traffic.json: round 6's instances carry one more template argument, the phase-stamp switch)
PMC_KERNEL = {
    ("conv2d_bwd_weight", 1024, 200, 200, 3, 32, 8, 4): ("conv1_wgrad_kernel<3, 2, false", "max"),
    ("conv2d_bwd_weight", 1024, 84, 84, 3, 32, 8, 4): ("conv1_wgrad_kernel<3, 2, false", "min"),
    ("conv2d_fwd", 1024, 200, 200, 3, 32, 8, 4): ("conv1_band_kernel<3, false, false>", "max"),
    ("conv2d_fwd", 1024, 84, 84, 3, 32, 8, 4): ("conv1_band_kernel<3, false, false>", "min"),
    ("conv2d_bwd_data", 2048, 49, 49, 32, 64, 4, 2): ("conv_band_glds_kernel<4, 2, 2, 2, true>", "max"),   # (round 4: the direct-to-LDS instance)
    ("conv2d_fwd", 2048, 49, 49, 32, 64, 4, 2): ("conv_band_kernel<32, 2, 4, 4, 2, 12, false, false,", "max"),
    ("conv2d_bwd_weight", 2048, 49, 49, 32, 64, 4, 2): ("conv_wgrad_band_kernel<32, 2, 4, 4, 2, false, 10, 5, 1, true", "max"),
    ("rnn_wavefront", 32, 64, 2048, 1): ("rnn_wavefront2_kernel<2048, true", "max"),
    ("rnn_wavefront", 32, 64, 2048, 0): ("rnn_wavefront2_kernel<2048, false", "max"),
    ("hulc_adam_step",): ("adam_kernel", "max"),
    ("hulc_adam_step_lo",): ("adam_kernel", "max"),
    # round 4: conv1 takes both modalities' frame tensors in one launch (hulc_conv_desc.x2): 2048 frames per launch
    ("conv2d_bwd_weight", 2048, 200, 200, 3, 32, 8, 4): ("conv1_wgrad_kernel<3, 2, false", "max"),
    ("conv2d_bwd_weight", 2048, 84, 84, 3, 32, 8, 4): ("conv1_wgrad_kernel<3, 2, false", "min"),
    ("conv2d_fwd", 2048, 200, 200, 3, 32, 8, 4): ("conv1_band_kernel<3, false, false>", "max"),
    ("conv2d_fwd", 2048, 84, 84, 3, 32, 8, 4): ("conv1_band_kernel<3, false, false>", "min"),
}


def pmc_traffic(key):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes of this same command
    (profiles/*_pmc_traffic.json: FETCH_SIZE and WRITE_SIZE collected in separate passes, FETCH_SIZE doubled per the gfx950 note of
    MI355X_MICROARCH.md).  bench.py cannot run the profiler on itself; None when no committed measurement names the kernel."""
    want = PMC_KERNEL.get(tuple(key))
    files = sorted((ROOT / "profiles").glob("*_pmc_traffic.json"))
    if not want or not files:
        return None
    hits = [rec["traffic_bytes"] for name, rec in json.loads(files[-1].read_text()).get("kernels", {}).items() if name.startswith(want[0])]
    if not hits:
        return None
    return round(max(hits) if want[1] == "max" else min(hits))


def cpu_baseline(seconds_budget=24.0):
    """oracle training step (fwd + bwd + Adam) on the host cores, B=4/modality, S=32, fp32 — timed twice, as SURVEY §8d asks: with 8
    threads (the reference's slurm allocation, slurm_scripts/slurm_training.py:22-26, and what the build container has) and with every
    core torch sees.  `value` is the better of the two (a baseline, not a target); both are reported."""
    n_all = torch.get_num_threads()
    # 8 (the reference's allocation), 32 (where torch's intra-op scaling of this batch usually peaks), the PHYSICAL cores, every hardware thread
    counts = sorted({min(8, n_all), min(32, n_all), _physical_cores(n_all), n_all})
    runs = []
    for n in counts:
        torch.set_num_threads(n)
        runs.append(_cpu_baseline_run(seconds_budget / len(counts), n))
    torch.set_num_threads(n_all)
    best = max(runs, key=lambda r: r["value"])
    return {**best, "runs": [{"cores": r["cores"], "value": r["value"]} for r in runs], "physical_cores": _physical_cores(n_all)}


def _physical_cores(default: int) -> int:
    """distinct (package, core) pairs of /proc/cpuinfo that this process may run on: torch's default thread count is the number of hardware
    THREADS, and the oracle at that count is oversubscribed (round 3: 2.4 sequences/s on 128 threads against 16.5 on 8)"""
    try:
        allowed = os.sched_getaffinity(0)
        pairs, cpu, phys = set(), None, 0
        for line in open("/proc/cpuinfo"):
            if line.startswith("processor"):
                cpu = int(line.split(":")[1])
            elif line.startswith("physical id"):
                phys = int(line.split(":")[1])
            elif line.startswith("core id") and cpu in allowed:
                pairs.add((phys, int(line.split(":")[1])))
        return max(1, min(len(pairs) or default, default))
    except Exception:                                       # noqa: BLE001
        return default


def _cpu_baseline_run(seconds_budget, threads):
    from hulc2_amd import param_spec, synthetic as syn
    from oracle import hulc2_oracle as O

    B, S = 4, 32
    torch.manual_seed(0)
    sd = {k: torch.empty(s) for k, s in param_spec.trainable_shapes().items()}
    syn.fill_state_dict_(sd, 42)
    for v in sd.values():
        v.requires_grad_(True)
    opt = torch.optim.Adam(list(sd.values()), lr=2e-4)
    raw = syn.make_batch(42, B, S)
    batch = {}
    for m, db in raw.items():
        batch[m] = dict(rgb_static=db["rgb_obs"]["rgb_static"], rgb_gripper=db["rgb_obs"]["rgb_gripper"], actions=db["actions"],
                        robot_obs=db["state_info"]["robot_obs"], plan_idx=db["plan_idx"])
        if m == "lang":
            batch[m].update(lang=db["lang"], use_for_aux_lang_loss=db["use_for_aux_lang_loss"])
    times = []
    t_start = time.time()
    for i in range(5):
        t0 = time.time()
        opt.zero_grad(set_to_none=True)
        out = O.training_step(sd, batch, dict(gripper_control=True))
        out["total_loss"].backward()
        opt.step()
        times.append(time.time() - t0)
        if time.time() - t_start > seconds_budget and i >= 1:
            break
    t = sorted(times[1:] or times)[len(times[1:] or times) // 2]
    return {"value": round(2 * B / t, 3), "unit": "play-sequences/s", "cores": threads, "kind": "port",
            "sample": f"{len(times)} steps of B={B}/modality S={S} (8 sequences/step; the GPU step is B=32/modality — the oracle's step "
                      f"time at that size does not fit the bench budget), fp32 torch CPU oracle, median of steps after the first"}


def cpu_baseline_affordance(seconds_budget=24.0):
    """the affordance oracle (frozen trunk restatement + decoder / head / depth step, fwd + bwd + Adam) on the host cores at B = 2, 224 x 224:
    8 threads and every core, as cpu_baseline() does"""
    from hulc2_amd import synthetic as syn
    from oracle import affordance_oracle as A

    def resnet18_shapes():                   # torchvision's resnet18 state_dict (conv / BatchNorm tensors of the stem and the 8 BasicBlocks)
        out = {"conv1.weight": (64, 3, 7, 7)}
        def bn(q, c):
            for leaf in ("weight", "bias", "running_mean", "running_var"):
                out[f"{q}.{leaf}"] = (c,)
        bn("bn1", 64)
        cin = 64
        for li, c in enumerate((64, 128, 256, 512), start=1):
            for b in range(2):
                q = f"layer{li}.{b}."
                out[q + "conv1.weight"] = (c, cin if b == 0 else c, 3, 3); bn(q + "bn1", c)
                out[q + "conv2.weight"] = (c, c, 3, 3); bn(q + "bn2", c)
                if b == 0 and li > 1:
                    out[q + "downsample.0.weight"] = (c, cin, 1, 1); bn(q + "downsample.1", c)
            cin = c
        return out

    B, HW = 2, 224
    sd = {k: torch.empty(s) for k, s in A.trainable_shapes(HW // 32).items()}
    syn.fill_affordance_state_dict_(sd, 42)
    tsd = {"r3m.convnet." + k: torch.empty(s) for k, s in resnet18_shapes().items()}
    syn.fill_state_dict_(tsd, 42)
    for v in sd.values():
        v.requires_grad_(True)
    opt = torch.optim.Adam(list(sd.values()), lr=1e-4)
    g = torch.Generator().manual_seed(0)
    img = torch.randn(B, 3, HW, HW, generator=g)
    emb = torch.randn(B, 384, generator=g) * 0.5
    p0 = torch.randint(0, HW, (B, 2), generator=g)
    depth = torch.randn(B, generator=g)
    n_all = torch.get_num_threads()
    runs = []
    for n in sorted({min(8, n_all), n_all}):
        torch.set_num_threads(n)
        times, t_start = [], time.time()
        for i in range(5):
            t0 = time.time()
            opt.zero_grad(set_to_none=True)
            with torch.no_grad():
                feats = A.trunk_maps(tsd, img)
            A.training_step(sd, feats, emb, p0, depth, HW)["loss"].backward()
            opt.step()
            times.append(time.time() - t0)
            if time.time() - t_start > seconds_budget / 2 and i >= 1:
                break
        t = sorted(times[1:] or times)[len(times[1:] or times) // 2]
        runs.append({"cores": n, "value": round(B / t, 3), "steps": len(times)})
    torch.set_num_threads(n_all)
    best = max(runs, key=lambda r: r["value"])
    return {"value": best["value"], "unit": "images/s", "cores": best["cores"], "kind": "port",
            "sample": f"{best['steps']} steps of B={B} images 224 x 224 (the GPU step is B=32), fp32 torch CPU oracle (trunk restatement + "
                      "oracle/affordance_oracle.py), median of steps after the first",
            "runs": [{"cores": r["cores"], "value": r["value"]} for r in runs]}


SECONDARY_NOTES = {
    "bf16+sites": ("bf16", "the bf16 step with every cheap exact-forward site on (HULC_FP32_SITES=head,goal,encfc,txl,conv1,a3: conv1 and the transformer "
                           "trunk from split bf16 operands, goal encoders / fc tails / contrastive head exact, the conv stacks' output map in fp32): "
                           "median gradient error 0.84 % against the fp32 oracle at full size, 10 of 106 tensors above 5 %, worst 10 % "
                           "(tests/test_parity_gpu.py::test_benchmarked_config_against_oracle[32-32-True-bf16+sites]); secondary, never the headline"),
    "bf16+a3": ("bf16", "the headline step + the site a3 (HULC_FP32_SITES=head,goal,encfc,txl,a3): the static camera's conv3 also stores an fp16 twin of "
                        "its output map (hulc_conv_desc.y_bf16 with an HULC_F16 output) for the spatial softmax.  The headline itself already runs the gripper "
                        "camera's exact-fp32 flatten-linear on an exact map (site encfc, round 6) — that operand's rounding was what held the FORWARD perceptual "
                        "embeddings at 1.06e-3; they measure 9.0e-4 against the fp32 oracle at full size now, with or without a3 "
                        "(tools/study/emb_error_sites.py); secondary, never the headline"),
    "fp32": ("f32", "exact fp32 MFMA compute + fp32 activations: the mode that meets 1e-3 element-wise parity; secondary, never the headline"),
    "mixed": ("bf16+f32", "exact-fp32 FORWARD upstream of the contrastive head (camera encoders, goal encoders, prior, posterior), bf16 backward and "
                          "bf16 recurrent decoder: every parameter gradient within 1.1 % of the fp32 oracle at full size (median 0.65 %) "
                          "(tests/test_parity_gpu.py::test_benchmarked_config_against_oracle[32-32-True-mixed]); secondary, never the headline"),
}


EXACT_SITES_ALL = "head,goal,encfc,txl,conv1,a3"


def secondary_mode(args, dev, mode):
    """The same step in another arithmetic mode (kernels.set_compute): 'fp32' = exact-fp32 MFMA everywhere (v_mfma_f32_32x32x2_f32, fp32
    storage: north_star's 1e-3 element-wise against the reference fixtures), 'mixed' = exact forward / bf16 backward (parity-grade GRADIENTS
    at bf16-class cost).  Reported next to the bf16 headline so the parity-grade modes have a throughput; never `value`."""
    from hulc2_amd import kernels as kn, synthetic as syn
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config
    from hulc2_amd.trainer import ArenaTrainer
    dtype, note = SECONDARY_NOTES[mode]
    sites_before = os.environ.get("HULC_FP32_SITES")
    try:
        if mode == "bf16+sites":           # the bf16 step with every cheap exact-forward site switched on
            os.environ["HULC_FP32_SITES"] = EXACT_SITES_ALL
        elif mode == "bf16+a3":            # the headline's sites + the static camera's finer conv3 map for the spatial softmax
            os.environ["HULC_FP32_SITES"] = "head,goal,encfc,txl,a3"
        kn.set_compute("bf16" if mode.startswith("bf16") else mode)
        model = instantiate(default_model_config(gripper_control=True, dropout_p=0.1)).to(dev)
        syn.fill_state_dict_(model.state_dict(), 42)
        model.train()
        tr = ArenaTrainer(model, lr=2e-4, overlap=False)
        batch = syn.make_batch(42, args.batch, args.seq_len, device=dev)
        for db in batch.values():
            db.pop("plan_idx", None)
        for i in range(2):
            tr.step(batch, i)
        tr.capture(batch)
        for _ in range(2):
            tr.replay()
        torch.cuda.synchronize()
        k = max(3, min(args.steps, 8 if mode == "fp32" else 20))
        t0 = time.perf_counter()
        for _ in range(k):
            loss = tr.replay()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        tr.close()
        return {"mode": mode, "dtype": dtype, "value": round(2 * args.batch * k / el, 2), "unit": "play-sequences/s", "ms_per_step": round(el / k * 1e3, 3),
                "steps": k, "final_loss": round(float(loss), 4), "note": note}
    except Exception as e:                                  # noqa: BLE001 - the headline line must still be printed
        return {"mode": mode, "dtype": dtype, "error": f"{type(e).__name__}: {e}"}
    finally:
        if sites_before is None:
            os.environ.pop("HULC_FP32_SITES", None)
        else:
            os.environ["HULC_FP32_SITES"] = sites_before
        kn.set_compute(args.compute)


def lightning_loop(args, dev):
    """The loop the reference's trainer actually drives (hulc2/training.py:79-82: Lightning -> training_step -> backward -> optimizer.step;
    conf/trainer/play_trainer.yaml:3 `precision: 16`): `model.training_step` inside torch.autocast(fp16), GradScaler.scale(loss).backward(),
    scaler.step(torch.optim.Adam), eager launches, no ArenaTrainer, no hipGraph — what a user gets who only swaps the class paths
    (INTEGRATION §1).  Two variants: the cooperative (device-wide barrier) kernels ON — one process, nothing else on the GPU — and with
    kernels.set_concurrent_streams(True), the setting torch's own DDP needs unless hulc2_amd.ddp.register_parked_comm_hook is used.
    Secondary, never `value`."""
    from hulc2_amd import kernels as kn, synthetic as syn
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config
    res = {"what": "Lightning-style loop: autocast(fp16) + GradScaler + model.training_step + loss.backward() + torch.optim.Adam.step(), no ArenaTrainer "
                   "(hulc2/training.py:79-82 with the class paths swapped, INTEGRATION §1); round 5: training_step is ONE autograd node, two replayed "
                   "hipGraphs from its third call on (hulc2_amd/stepnode.py); `cooperative_kernels_no_step_node` = round 4's loop", "unit": "play-sequences/s"}
    try:
        kn.set_compute("bf16")
        model = instantiate(default_model_config(gripper_control=True, dropout_p=0.1)).to(dev)
        syn.fill_state_dict_(model.state_dict(), 42)
        model.train()
        batch = syn.make_batch(42, args.batch, args.seq_len, device=dev)
        for db in batch.values():
            db.pop("plan_idx", None)
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=2e-4)
        scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)

        def step(i):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16):
                loss = model.training_step(batch, i)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            return loss

        def measure(name):
            for i in range(3):
                loss = step(i)
            torch.cuda.synchronize()
            k = max(3, min(args.steps, 20))
            t0 = time.perf_counter()
            for i in range(k):
                loss = step(i)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            kn.check_faults(dev)
            res[name] = {"value": round(2 * args.batch * k / el, 2), "ms_per_step": round(el / k * 1e3, 3), "steps": k,
                         "final_loss": round(float(loss), 4)}

        def node_stats(name):
            node = model.__dict__.get("_hulc_step_node")
            if node is not None:
                res[name]["step_node"] = {"replays": node.replays, "eager_steps": node.eager_steps, "captures": node.captures,
                                          "input_copies": node.input_copies, "accum_steps": node.accum_steps, "zeroed_steps": node.zeroed_steps,
                                         "disabled": node.disabled}

        for name, conc in (("cooperative_kernels", False), ("concurrent_streams", True)):
            kn.set_concurrent_streams(conc)
            measure(name)
            node_stats(name)
        # the same loop with ONE class path more swapped: `optimizer._target_: hulc2_amd.optim.Adam` (torch.optim.Adam's rule and state_dict; the step
        # is the arena launch that also writes the kernel-side weight copies — torch's multi-tensor step costs ~1.5 ms of host time here)
        from hulc2_amd.optim import Adam as HulcAdam
        kn.set_concurrent_streams(False)
        torch_opt = opt
        opt = HulcAdam([p for p in model.parameters() if p.requires_grad], lr=2e-4)
        opt.load_state_dict(torch_opt.state_dict())
        measure("cooperative_kernels_hulc2_amd_adam")
        res["cooperative_kernels_hulc2_amd_adam"]["fused_steps"] = int(opt.fused_launches)
        node_stats("cooperative_kernels_hulc2_amd_adam")
        # a data loader delivers every batch at NEW addresses: the node copies it into the graphs' input buffers (1.16 GB of frames per step).
        # Two more resident batches, alternated: every step pays the copy
        try:
            others = [syn.make_batch(43 + j, args.batch, args.seq_len, device=dev) for j in range(2)]
            for b2 in others:
                for db in b2.values():
                    db.pop("plan_idx", None)

            def step(i):                                    # noqa: F811
                opt.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.float16):
                    loss = model.training_step(others[i % 2], i)
                scaler.scale(loss).backward()
                scaler.step(opt)
                scaler.update()
                return loss
            measure("hulc2_amd_adam_batches_at_new_addresses")
            node_stats("hulc2_amd_adam_batches_at_new_addresses")
        except Exception as e:                              # noqa: BLE001
            res["new_addresses_error"] = f"{type(e).__name__}: {e}"
        finally:
            del others

            def step(i):                                    # noqa: F811
                opt.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.float16):
                    loss = model.training_step(batch, i)
                scaler.scale(loss).backward()
                scaler.step(opt)
                scaler.update()
                return loss
        # round 6: (a) the optimizer the UNCHANGED conf/model/optimizer/adam.yaml gets from Hulc2.configure_optimizers (`_target_: torch.optim.Adam`
        # -> the drop-in subclass), (b) in the order pytorch-lightning 1.8's closure runs a step — training_step -> optimizer.zero_grad() -> backward —
        # with the previous step's .grad still attached while training_step runs, set_to_none as torch 2.x defaults (True) and as the torch 1.12 the
        # reference pins defaults (False: zeroed in place, still attached at backward time -> the node's add-back path, stepnode._take_live_grads)
        try:
            hulc_opt = opt
            opt = model.configure_optimizers()["optimizer"]
            res["configure_optimizers_class"] = f"{type(opt).__module__}.{type(opt).__name__}"
            opt.load_state_dict(hulc_opt.state_dict())
            for name, stn in (("default_yaml_lightning_closure_order", True), ("default_yaml_lightning_closure_order_zero_in_place", False)):
                def step(i, stn=stn):                       # noqa: F811
                    with torch.autocast("cuda", dtype=torch.float16):
                        loss = model.training_step(batch, i)
                    opt.zero_grad(set_to_none=stn)
                    scaler.scale(loss).backward()
                    scaler.step(opt)
                    scaler.update()
                    return loss
                node = model.__dict__.get("_hulc_step_node")
                before = (node.replays, node.accum_steps, node.zeroed_steps) if node is not None else (0, 0, 0)
                measure(name)
                node_stats(name)
                if node is not None:
                    res[name]["replays_in_this_leg"] = node.replays - before[0]
                    res[name]["accum_steps_in_this_leg"] = node.accum_steps - before[1]
                    res[name]["zeroed_steps_in_this_leg"] = node.zeroed_steps - before[2]   # (arena zeroed by optim.Adam.zero_grad: no add-back)
                res[name]["fused_steps"] = int(getattr(opt, "fused_launches", -1))
        except Exception as e:                              # noqa: BLE001
            res["closure_order_error"] = f"{type(e).__name__}: {e}"
        finally:
            def step(i):                                    # noqa: F811
                opt.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.float16):
                    loss = model.training_step(batch, i)
                scaler.scale(loss).backward()
                scaler.step(opt)
                scaler.update()
                return loss
        opt = torch_opt
        # the same loop under torch's own DistributedDataParallel (what Lightning's DDPStrategy builds, hulc2/training.py:72-75), on a ONE-rank
        # RCCL group — the collectives move nothing, the reducer's bucket copies, hooks and stream hand-overs are all there: with
        # hulc2_amd.ddp.register_parked_comm_hook (cooperative kernels stay on, bucket all-reduces parked behind the last cooperative kernel of
        # the backward) and with torch's default hook + set_concurrent_streams(True) (round 3's only option under DDP)
        own_group = False
        try:
            from torch.nn.parallel import DistributedDataParallel as DDP
            from hulc2_amd.ddp import register_parked_comm_hook
            if not dist.is_initialized():
                dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=dev)
                own_group = True

            class _Step(torch.nn.Module):               # Lightning's _LightningModuleWrapperBase: forward = training_step
                def __init__(self, m):
                    super().__init__()
                    self.module = m

                def forward(self, b, i):
                    return self.module.training_step(b, i)

            # (`_one_bucket`: gradient_as_bucket_view=True + one 200 MB bucket — the reducer copies every gradient into ONE buffer and hands the
            #  views back as .grad: no per-bucket launches, no copy back; `_hulc2_amd_adam`: the optimizer configure_optimizers now returns)
            for name, conc, parked, extra, hulc_adam in (("torch_ddp_parked_hook", False, True, {}, False),
                                                         ("torch_ddp_parked_hook_one_bucket", False, True, dict(gradient_as_bucket_view=True, bucket_cap_mb=200), False),
                                                         ("torch_ddp_parked_hook_one_bucket_hulc2_amd_adam", False, True, dict(gradient_as_bucket_view=True, bucket_cap_mb=200), True),
                                                         ("torch_ddp_parked_hook_hulc2_amd_adam", False, True, {}, True),
                                                         ("torch_ddp_concurrent_streams", True, False, {}, False)):
                kn.set_concurrent_streams(conc)
                if hulc_adam:
                    opt = HulcAdam([p for p in model.parameters() if p.requires_grad], lr=2e-4)
                    opt.load_state_dict(torch_opt.state_dict())
                else:
                    opt = torch_opt
                ddp = DDP(_Step(model), device_ids=[dev.index or 0], static_graph=True, find_unused_parameters=False, **extra)
                if parked:
                    register_parked_comm_hook(ddp)
                inner_step = step

                def step(i, ddp=ddp):                   # noqa: F811 - the same loop, the module called through DDP
                    opt.zero_grad(set_to_none=True)
                    with torch.autocast("cuda", dtype=torch.float16):
                        loss = ddp(batch, i)
                    scaler.scale(loss).backward()
                    scaler.step(opt)
                    scaler.update()
                    return loss
                try:
                    measure(name)
                    node_stats(name)
                finally:
                    step = inner_step
                    opt = torch_opt
                    del ddp
        except Exception as e:                              # noqa: BLE001
            res["torch_ddp_error"] = f"{type(e).__name__}: {e}"
        finally:
            if own_group and dist.is_initialized():
                dist.destroy_process_group()
        # round 4's loop for comparison: the step as ~160 autograd Functions instead of ONE node (HULC_NO_STEP_NODE=1; a fresh model: the
        # keeper of the first one owns a gradient arena and the node)
        had = os.environ.get("HULC_NO_STEP_NODE")
        os.environ["HULC_NO_STEP_NODE"] = "1"
        try:
            kn.set_concurrent_streams(False)
            del model, opt, torch_opt
            model = instantiate(default_model_config(gripper_control=True, dropout_p=0.1)).to(dev)
            syn.fill_state_dict_(model.state_dict(), 42)
            model.train()
            opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=2e-4)
            measure("cooperative_kernels_no_step_node")
        except Exception as e:                              # noqa: BLE001
            res["no_step_node_error"] = f"{type(e).__name__}: {e}"
        finally:
            if had is None:
                os.environ.pop("HULC_NO_STEP_NODE", None)
            else:
                os.environ["HULC_NO_STEP_NODE"] = had
    except Exception as e:                                  # noqa: BLE001 - the headline line must still be printed
        res["error"] = f"{type(e).__name__}: {e}"
    finally:
        kn.set_concurrent_streams(False)
        kn.set_compute(args.compute)
    return res


def roofline_leg(args, trainer, model, batch, dev, peak):
    """--full: per-launch HIP events on the launch stream over 3 more eager steps (outside the timed region) -> (the per-kernel table, the
    dominant kernel's roofline entry, the transformer trunk's entry or None).
    The dominant kernel = the (entry point, shape) with the largest summed time.  Its bound is whichever roof needs longer for
    the launch's ALGORITHMIC work (kernels.py annotates flops = 2 x MACs and bytes = every operand / result touched once):
    bytes / 8 TB/s vs flops / dense MFMA peak.  achieved = that work / the measured average launch duration.
    (one stream for this leg: with the camera encoders on two streams the gripper camera's kernels run INSIDE the static camera's launches and
    every per-launch duration would include its neighbour's share of the chip)"""
    from hulc2_amd import kernels as kn
    prev_streams, prev_fork = os.environ.get("HULC_ENC_STREAMS"), os.environ.get("HULC_FORK")
    os.environ["HULC_ENC_STREAMS"] = "0"
    os.environ["HULC_FORK"] = "0"                           # (round 6: one chain here — the forked branches overlap launches; the timed region ran the forked graph)
    trainer.step(batch, 0)                                  # untimed: the one-chain arrangement's per-stream workspaces exist before the timed launches (a first use read 238 us for the trunk's backward instead of 117)
    kn.start_timing()
    for i in range(3):
        trainer.step(batch, i)
    table = kn.stop_timing()
    for k_, v_ in (("HULC_ENC_STREAMS", prev_streams), ("HULC_FORK", prev_fork)):
        if v_ is None:
            os.environ.pop(k_, None)
        else:
            os.environ[k_] = v_
    total_ms = sum(v[1] for v in table.values())
    dom_key, (dom_n, dom_t, dom_flops, dom_bytes) = max(table.items(), key=lambda kv: kv[1][1])
    avg_s = dom_t / dom_n * 1e-3
    hbm_bound = dom_bytes / PEAK_HBM >= dom_flops / peak
    if hbm_bound:
        rl = {"bound": "hbm", "achieved": round(dom_bytes / avg_s / 1e9, 1), "peak": PEAK_HBM / 1e9, "unit": "GB/s",
              "frac": round(dom_bytes / avg_s / PEAK_HBM, 4)}
    else:
        rl = {"bound": "mfma", "achieved": round(dom_flops / avg_s / 1e12, 2), "peak": peak / 1e12, "unit": "TFLOP/s",
              "frac": round(dom_flops / avg_s / peak, 4)}
    rl["traffic"] = pmc_traffic(dom_key)
    rl.update({"kernel": "/".join(str(k) for k in dom_key),
               "algorithmic_bytes_per_launch": dom_bytes, "algorithmic_flops_per_launch": dom_flops,
               "launches_per_step": dom_n // 3, "avg_launch_ms": round(dom_t / dom_n, 4),
               "kernel_share_of_step": round(dom_t / max(total_ms, 1e-9), 3),
               "gpu_kernel_ms_per_step": round(total_ms / 3, 3)})
    rl_txl = None
    if not (args.affordance or args.real_world) and args.compute == "bf16":
        try:
            rl_txl = txl_roofline(table, model, dev, peak, 2 * args.batch, alone=not args.no_secondary)
        except Exception as e:                              # noqa: BLE001
            rl_txl = {"error": f"{type(e).__name__}: {e}"}
    return table, rl, rl_txl


TXL_FLOP_PER_SEQ = 229.6e6        # the two transformer layers, forward + backward, per 32-step play sequence (2 x 598 016 MAC per token and layer)


def txl_roofline(table, model, dev, peak, seqs_in_step, alone=True):
    """north_star's one explicit kernel target (>= 60 % of the MFMA roof on the transformer block) as numbers in the line: the posterior's trunk
    launches (csrc/txl_block.hip: one launch per direction) inside the step — from the same HIP-event leg as `roofline` — and the same two
    launches alone at 256 and 1024 sequences, where the launch is no longer latency-bound (the kernel's asymptotic MFMA fraction next to the
    64-sequence figure).  flops = sequences x 229.6 MFLOP (algorithmic), frac = flops / (fwd + bwd time) / dense bf16 MFMA peak."""
    from hulc2_amd import kernels as kn

    def pick(tbl, B):
        us = {}
        for k, (n, t, _, _) in tbl.items():
            if k[0] in ("txl_block_fwd", "txl_block_bwd") and k[1] == B and n:
                us[k[0]] = t / n * 1e3
        return us

    def entry(B, us):
        if len(us) != 2:
            return {"sequences": B, "error": "the whole-trunk launches did not run (per-layer path)"}
        tot = us["txl_block_fwd"] + us["txl_block_bwd"]
        fl = B * TXL_FLOP_PER_SEQ
        return {"sequences": B, "fwd_us": round(us["txl_block_fwd"], 1), "bwd_us": round(us["txl_block_bwd"], 1), "flops": fl,
                "achieved_tflops": round(fl / (tot * 1e-6) / 1e12, 1), "frac": round(fl / (tot * 1e-6) / peak, 4)}

    out = {"bound": "mfma", "peak": peak / 1e12, "unit": "TFLOP/s", "in_step": entry(seqs_in_step, pick(table, seqs_in_step)), "alone": []}
    net = getattr(model, "plan_recognition", None)
    if net is None or not alone:                            # (--no-secondary: profiling runs keep the step's own launches only)
        return out
    for B in (256, 1024):
        try:
            emb = torch.randn(B, 32, 128, device=dev, requires_grad=True)
            for _ in range(2):
                st, feat = net(emb)
                (st.logit.sum() + feat.sum()).backward()
            kn.start_timing()
            for _ in range(5):
                st, feat = net(emb)
                (st.logit.sum() + feat.sum()).backward()
            out["alone"].append(entry(B, pick(kn.stop_timing(), B)))
        except Exception as e:                              # noqa: BLE001 - a secondary figure must not cost the headline line
            out["alone"].append({"sequences": B, "error": f"{type(e).__name__}: {e}"})
    for prm in net.parameters():
        prm.grad = None
    return out


DUMP_SAMPLE = 16384               # --dump-outputs: elements kept per tensor (108 parameters + their gradients: at most 14 MB in all)


def dump_outputs(path, model, loss) -> None:
    """What the timed path hands its caller after its last step: the loss, every trainable parameter after the optimizer update and the
    gradient that update consumed, as float32 / float64 .npy files.  A tensor of more than DUMP_SAMPLE elements is written as a fixed
    sample: the indices come from a generator seeded with the tensor's name, so two builds compare element for element."""
    import zlib

    import numpy as np
    out = Path(path)
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / "loss.npy", np.array([float(loss)], dtype=np.float64))
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        for kind, t in (("param", p), ("grad", p.grad)):
            if t is None:
                continue
            flat = t.detach().reshape(-1)
            if flat.numel() > DUMP_SAMPLE:
                idx = np.random.RandomState(zlib.crc32(name.encode())).randint(0, flat.numel(), DUMP_SAMPLE)
                flat = flat[torch.from_numpy(idx).to(flat.device)]
            np.save(out / f"{kind}.{name}.npy", flat.float().cpu().numpy())


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` from a plain shell: start N rank processes (one per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set
    as torch.distributed.run would) and relay rank 0's JSON line.  The parent never touches the GPU (no HIP call, no torch.cuda query
    beyond device_count) and never execs: the ranks are fresh child processes.  What Lightning's DDPStrategy launcher does for the
    reference (hulc2/training.py:72-75,122-145)."""
    import subprocess
    import tempfile

    backend = os.environ.get("HULC_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()                       # counts devices without creating a HIP context
    if backend == "nccl" and ndev < n and "--dry-run" not in sys.argv:
        print(f"[bench] --gpus {n} needs {n} GPUs for the RCCL backend, this node shows {ndev} "
              f"(HULC_BENCH_BACKEND=gloo shares devices for a functional check)", file=sys.stderr)
        return 2
    port = _free_port()
    procs, outs = [], []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        out = tempfile.TemporaryFile(mode="w+") if r == 0 else subprocess.DEVNULL
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env, stdout=out))
    rc = 0
    limit = float(os.environ.get("HULC_BENCH_LIMIT_S", "1500"))       # all ranks stuck (a collective nobody completes): give up instead of waiting forever
    t_start = time.time()
    while any(p.poll() is None for p in procs):
        if time.time() - t_start > limit:
            print(f"[bench] the ranks did not finish within {limit:.0f} s (HULC_BENCH_LIMIT_S): ending them", file=sys.stderr)
            rc = 124
            for p in procs:
                if p.poll() is None:
                    p.terminate()                          # exactly the PIDs started above
            break
        bad = [p for p in procs if p.poll() not in (None, 0)]
        if bad:                                            # one rank died: the others would wait in a collective forever
            rc = bad[0].returncode or 1
            for p in procs:
                if p.poll() is None:
                    p.terminate()                          # exactly the PIDs started above
            break
        time.sleep(0.2)
    for p in procs:
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()
        if p.returncode not in (0, None) and rc == 0:
            rc = p.returncode
    outs[0].seek(0)
    for line in outs[0].read().splitlines():               # stdout carries the ONE JSON line; library chatter (gloo prints there) goes to stderr
        print(line, file=sys.stdout if line.lstrip().startswith("{") else sys.stderr)
    sys.stdout.flush()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100, help="timed steps (default 100: a 0.4 s timed region; 20 steps were 75 ms, inside the box-to-box noise)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32, help="play sequences per modality per GPU")
    ap.add_argument("--seq-len", type=int, default=32)
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32", "mixed"])
    ap.add_argument("--full", action="store_true",
                    help="after the headline: the per-kernel roofline leg, the secondary arithmetic modes and the Lightning-style loop (unless "
                         "--no-secondary) and the CPU baseline (unless --no-cpu-baseline); a plain run measures the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed (loss, parameters after the update, their gradients; a fixed sample of "
                         "large tensors) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying captured HIP graphs")
    ap.add_argument("--breakdown", action="store_true", help="print the per-kernel time table to stderr (runs the roofline leg, as --full does)")
    ap.add_argument("--affordance", action="store_true", help="BASELINE configs[4] (secondary): one training step of the affordance model "
                    "(PixelAffLangDetector, r3m variant) on --batch images of 224 x 224; the metric becomes images per second")
    ap.add_argument("--trunk-mode", default="frozen", choices=["frozen", "reference"],
                    help="--affordance: 'frozen' = inference-mode trunk (default), 'reference' = the trunk's BatchNorms on batch statistics as the "
                         "reference's training loop runs them (hulc2/affordance/models/visual_lang_encoders/r3m_rn18.py:27-43)")
    ap.add_argument("--uint8-frames", action="store_true",
                    help="feed uint8 NHWC frames + shift-augmentation offsets (SURVEY 8 row f-2) instead of transformed fp32 frames; "
                         "a separate data format, not the headline configuration")
    ap.add_argument("--episode-store", action="store_true",
                    help="row f-2 end to end: an HBM-resident uint8 episode store per modality, every step draws new play windows "
                         "(index rows, pad-by-repetition, shifts) and conv1 reads the store in place; separate from the headline configuration")
    ap.add_argument("--store-frames", type=int, default=16384, help="frames in the synthetic episode store (141 KB each)")
    ap.add_argument("--real-world", action="store_true",
                    help="secondary measurement, BASELINE configs[3] (cfg_low_level_rw): static camera 150x200 in [0,255] through the frozen R3M "
                         "ResNet-18 trunk, whole-embedding decoder input, world-frame actions, no CLIP loss")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the fp32-compute (1e-3 parity mode) throughput leg")
    ap.add_argument("--force-dist", action="store_true",
                    help="with one rank: still create the process group and run the multi-rank control flow (split graphs, comm stream, "
                         "collectives) — executes the RCCL path on a one-GPU box")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch check only: every rank joins a gloo process group on the CPU, all-reduces one number and rank 0 prints "
                         "n_ranks_seen — no GPU work (diagnoses the --gpus N launcher on any machine)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # stdout carries the ONE JSON line and nothing else: RCCL prints a five-line version banner to the C stdout of every process that creates a
    # communicator (and gloo its own chatter), flushed at exit — i.e. AFTER the line.  From here on file descriptor 1 is stderr; the line is
    # written to the saved descriptor.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    def emit(obj) -> None:
        os.write(real_stdout, (json.dumps(obj) + "\n").encode())

    if args.dry_run:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([float(rank + 1)])
        dist.all_reduce(t)
        if rank == 0:
            emit({"dry_run": True, "n_gpus": world, "n_ranks_seen": dist.get_world_size(), "rank_sum": t.item(), "gpus_flag": args.gpus})
        dist.destroy_process_group()
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    # HULC_BENCH_BACKEND=gloo: functional check of the multi-rank control flow on a box with fewer GPUs than ranks (ranks then share devices;
    # the device-wide-barrier kernels need the GPU to themselves and are switched off then).  The measured configuration is nccl (= RCCL).
    backend = os.environ.get("HULC_BENCH_BACKEND", "nccl")
    if backend != "nccl" and world > torch.cuda.device_count():
        os.environ["HULC_NO_RNN_WAVEFRONT"] = os.environ["HULC_NO_MLP_CHAIN"] = "1"
    dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world != args.gpus and rank == 0:
        print(f"[bench] --gpus {args.gpus} but WORLD_SIZE={world}: the launcher's world size wins", file=sys.stderr)
    force_dist = args.force_dist or bool(os.environ.get("HULC_BENCH_FORCE_DIST"))
    if world > 1 or force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            os.environ["MASTER_PORT"] = str(_free_port())
        import datetime
        kw = dict(rank=rank, world_size=world, timeout=datetime.timedelta(seconds=float(os.environ.get("HULC_BENCH_DIST_TIMEOUT_S", "600"))))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, **kw)
        else:
            dist.init_process_group(backend, **kw)

    from hulc2_amd import kernels as kn, synthetic as syn
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config, real_world_model_config
    from hulc2_amd.trainer import ArenaTrainer

    kn.set_compute(args.compute)
    if args.real_world and (args.uint8_frames or args.episode_store):
        raise SystemExit("--real-world takes fp32 frames in [0,255] (conf/datamodule/transforms/real_world_r3m.yaml); the uint8 store feeds the CNN config")
    use_graph = not args.no_graph
    if args.affordance:
        from hulc2_amd.affordance import PixelAffLangDetector
        model = PixelAffLangDetector(img_size=224, trunk_mode=args.trunk_mode).to(dev)
        syn.fill_affordance_state_dict_({k: v for k, v in model.state_dict().items() if ".r3m." not in k}, 42)
        syn.fill_state_dict_({"r3m.convnet." + k: v for k, v in model.model.aff_stream.r3m.convnet.state_dict().items()}, 42)
        model.train()
        trainer = ArenaTrainer(model, lr=1e-4, overlap=not use_graph, force_comm=force_dist)
        g = torch.Generator().manual_seed(42 + rank)
        nb = args.batch
        batch = ({"img": torch.randn(nb, 3, 224, 224, generator=g).to(dev), "lang_goal": (torch.randn(nb, 384, generator=g) * 0.5).to(dev)},
                 {"p0": torch.stack([torch.randint(0, 224, (nb,), generator=g), torch.randint(0, 224, (nb,), generator=g)], 1).to(dev),
                  "normalized_depth": torch.randn(nb, generator=g).to(dev)})
    else:
        cfg = real_world_model_config(dropout_p=0.1) if args.real_world else default_model_config(gripper_control=True, dropout_p=0.1)
        model = instantiate(cfg).to(dev)
        syn.fill_state_dict_(model.state_dict(), 42)            # same weights on every rank
        model.train()
        trainer = ArenaTrainer(model, lr=2e-4, overlap=not use_graph, force_comm=force_dist)
        batch = syn.make_batch(42 + rank, args.batch, args.seq_len, device=dev, **({"static_hw": (150, 200)} if args.real_world else {}))
    for db in ({} if args.affordance else batch).values():
        db.pop("plan_idx", None)                            # benchmark samples the latent plan on-device
        if args.real_world:                                 # UpScaleImageTensor: the R3M trunk takes [0, 255]
            db["rgb_obs"]["rgb_static"] = (db["rgb_obs"]["rgb_static"] + 1) * 127.5
    if args.uint8_frames:
        g = torch.Generator().manual_seed(1234 + rank)
        for db in batch.values():
            obs = {}
            for key, hw, pad in (("rgb_static", 200, 10), ("rgb_gripper", 84, 4)):
                obs[key] = torch.randint(0, 256, (args.batch, args.seq_len, hw, hw, 3), generator=g, dtype=torch.uint8).to(dev)
                obs[key + "_shift"] = torch.randint(0, 2 * pad + 1, (args.batch, args.seq_len, 2), generator=g, dtype=torch.int32).to(dev)
            db["rgb_obs"] = obs

    stores, draw = None, None
    if args.episode_store:
        import numpy as np
        from hulc2_amd.datasets import DeviceEpisodeStore
        g = torch.Generator().manual_seed(99 + rank)
        n = args.store_frames
        rgb = {"rgb_static": torch.randint(0, 256, (n, 200, 200, 3), generator=g, dtype=torch.uint8).to(dev),
               "rgb_gripper": torch.randint(0, 256, (n, 84, 84, 3), generator=g, dtype=torch.uint8).to(dev)}
        act = torch.rand(n, 7, generator=g) * 2 - 1
        act[:, 6] = torch.where(act[:, 6] > 0, 1.0, -1.0)
        obs = torch.randn(n, 15, generator=g)
        obs[:, 3:6] = (torch.rand(n, 3, generator=g) * 2 - 1) * 3.14159 * 0.5
        eps = [(a, min(a + 511, n - 1)) for a in range(0, n, 512)]           # 512-frame play episodes
        # vision windows 20..32 (conf/datamodule/datasets/vision_dataset/vision_shm.yaml:5-6); language windows 20..32 over 64-frame
        # annotated spans in the auto_lang_ann.npy layout, aux-loss window 8 (lang_dataset/lang_shm.yaml:5-6,12)
        stores = {"vis": DeviceEpisodeStore(rgb, act, obs, eps, 20, 32, device=dev, seed=rank)}
        spans = [(a + 64 * j, a + 64 * j + 63) for a, b in eps for j in range(0, (b - a + 1) // 64, 2)]
        lang_data = {"language": {"ann": [""] * len(spans), "task": [""] * len(spans),
                                  "emb": (torch.randn(len(spans), 1, 384, generator=g) * 0.05).numpy()}, "info": {"indx": spans}}
        stores["lang"] = DeviceEpisodeStore.from_language_annotations(stores["vis"].rgb, act, obs, lang_data, device=dev, seed=rank)
        sampler = np.random.RandomState(1000 + rank)

        def draw():
            for mod, st in stores.items():
                fresh = st.batch(sampler.randint(0, len(st), args.batch))
                fresh.pop("window_sizes")
                batch[mod] = fresh                                            # same device buffers every step: graph replay sees the new windows
        draw()

    def sync():
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    loss = None
    if use_graph:
        for i in range(2):                                  # eager steps: allocator pools + lazy buffers before capture
            loss = trainer.step(batch, i)
        try:
            trainer.capture(batch)
        except Exception as e:                              # noqa: BLE001 - report and fall back to eager launches
            print(f"[bench] graph capture failed ({type(e).__name__}: {e}); running eagerly", file=sys.stderr)
            use_graph = False
        if dist.is_initialized():                           # graph and eager modes issue different collectives: all ranks take the same one
            ok = torch.tensor([1 if use_graph else 0], device=dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            use_graph = bool(ok.item())
    run_step = (lambda i: trainer.replay()) if use_graph else (lambda i: trainer.step(batch, i))
    if draw is not None:
        inner = run_step

        def run_step(i):
            draw()
            return inner(i)
    for i in range(args.warmup):
        loss = run_step(i)
    comm_info = None
    if dist.is_initialized() and hasattr(trainer, "comm_exposed_ms"):
        trainer.comm_exposed_ms()                           # drop warm-up events
        trainer.time_comm = True                            # one event pair per step around the wait for the gradient exchange
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = run_step(i)
    sync()
    elapsed = time.perf_counter() - t0
    if dist.is_initialized():
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        if hasattr(trainer, "comm_exposed_ms"):
            # what an N-GPU number is made of: the bytes each rank exchanges per step, the algorithm (and the probe that picked it), and the
            # time per step the compute stream sat waiting for the exchange — the part of the all-reduce NOT hidden under the conv backward
            trainer.time_comm = False
            ex = torch.tensor([trainer.comm_exposed_ms()], device=dev, dtype=torch.float64)
            dist.all_reduce(ex, op=dist.ReduceOp.MAX)
            comm_info = dict(trainer.comm.describe(), comm_exposed_ms=round(float(ex.item()), 4),
                             overlap="split graphs: exchange of everything but the camera encoders' gradients runs under the conv backward graph"
                             if getattr(trainer, "graph_enc", None) is not None else
                             ("bucket hooks overlapped with backward" if not use_graph else "none (one graph, exchange between backward and optimizer)"))
    final_loss = float(loss)
    kn.check_faults(dev)                                    # a barrier-kernel timeout inside the timed region ends the run (non-zero exit), not a NaN line
    if final_loss != final_loss:
        raise SystemExit("[bench] the loss is NaN after the timed region")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, loss)        # before anything else steps the model

    rl = rl_txl = None
    peak = PEAK_F32 if args.compute == "fp32" else PEAK_BF16
    if args.full or args.breakdown:
        table, rl, rl_txl = roofline_leg(args, trainer, model, batch, dev, peak)
        if args.breakdown and rank == 0:
            rows = int(os.environ.get("HULC_BREAKDOWN_ROWS", "25"))
            for key, (n, t, f, b) in sorted(table.items(), key=lambda kv: -kv[1][1])[:rows]:
                a = t / n * 1e-3
                print(f"  {t / 3:9.3f} ms/step  {n // 3:4d} launches  {f / a / 1e12:8.1f} TFLOP/s  {b / a / 1e9:8.0f} GB/s  {key}", file=sys.stderr)
            print(f"  sum of kernel time: {rl['gpu_kernel_ms_per_step']:.3f} ms/step", file=sys.stderr)

    seqs = (1 if args.affordance else 2) * args.batch * world * args.steps
    ms_per_step = elapsed / args.steps * 1e3
    value = seqs / elapsed
    # real-world config: frozen trunk forward only (1 167 MMAC per 150x200 frame, by closed form over the 20 convolutions) + 3x the trained part
    seq_flop = (2 * 1167.0e6 * 32 + 3 * 2 * (237.37 + 59.24 + 15.01 + 4.78 + 492.2 + 0.15) * 1e6) if args.real_world else SEQ_FLOP_TRAIN
    if args.affordance:
        # per image: frozen ResNet-18 trunk forward (1.82 GMAC at 224 x 224) + 3 x the trainable part (decoder convolutions 6 256 MMAC by closed
        # form over unet_decoder.py's ten 3 x 3 layers and the head, depth / text MLPs 21 MMAC)
        seq_flop = 2 * 1.82e9 + 3 * 2 * (6256.0 + 21.0) * 1e6
        if args.trunk_mode == "reference":                 # + the trunk's data gradient (all layers but the stem) and the stem's weight gradient
            seq_flop += 2 * (1.82e9 - 0.118e9) + 2 * 0.118e9
    workload = ("BASELINE configs[4] (secondary): affordance model PixelAffLangDetector.training_step, shipped r3m variant — frozen R3M ResNet-18 trunk "
                + ("(random weights, trunk_mode=frozen: inference-mode BatchNorm folded into the convolutions)" if args.trunk_mode == "frozen" else
                   "(random weights, trunk_mode=reference: every trunk BatchNorm on BATCH statistics with running statistics updated, as the "
                   "reference's train() leaves them — r3m_rn18.py:27-43; STEM TRAINABLE as in the reference: conv1.weight / bn1 receive their gradient "
                   "through the data gradient of the whole frozen ResNet-18, hulc2_amd/affordance/trunk.py)")
                + ", language-fused U-Net decoder with BatchNorm on batch statistics, pixel cross-entropy + "
                "Gaussian depth NLL, Adam lr 1e-4; 224 x 224 images, lang = random (B,384) embeddings"
                if args.affordance else
                "BASELINE configs[3] (secondary): cfg_low_level_rw — static 150x200 in [0,255] through the frozen R3M ResNet-18 trunk (random "
                "weights), gripper CNN 84x84, decoder on the whole embedding, world-frame actions, no CLIP loss, lang = random (B,384) embeddings"
                if args.real_world else
                "BASELINE configs[1]: synthetic CALVIN-shaped batch, Hulc2.training_step fwd+bwd+allreduce+Adam, "
                "static CNN 200x200 + gripper CNN 84x84, lang = random (B,384) embeddings, dropout 0.1, gripper_control on")
    step_frac = round(value / world * seq_flop / peak, 4)
    out = {
        "metric": "affordance-images/sec/node (224x224, r3m variant)" if args.affordance
                  else "play-sequences/sec/node (seq_len=32, real-world cfg: R3M static 150x200)" if args.real_world
                  else "play-sequences/sec/node (seq_len=32, 200x200 RGB)",
        "value": round(value, 2), "unit": "images/s" if args.affordance else "play-sequences/s", "n_gpus": world,
        "n_ranks_seen": dist.get_world_size() if dist.is_initialized() else 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": {"bf16": "bf16", "fp32": "f32", "mixed": "bf16+f32"}[args.compute], "data": "synthetic",
        "config": {"workload": workload,
                   "sequences_per_gpu_step": (1 if args.affordance else 2) * args.batch, "seq_len": args.seq_len, "parallelism": f"dp{world}",
                   "launch": "hipGraph replay (fwd+bwd graph, all-reduce, optimizer graph)" if use_graph else "eager launches",
                   # round 6: independent branches of the step as branches of the captured graph (HULC_FORK=0: one chain, as until round 5)
                   "graph_branches": ("camera encoders x 2; posterior (transformer trunk + head) || goal encoders + prior, forward and backward, each on half "
                                      "of the device (hulc_set_coop_share 2); contrastive head || sample / KL / decoder projections"
                                      + ("; recurrent weight gradients || data-gradient chain" if kn.wgrad_branch_ok() or os.environ.get("HULC_WGRAD_FORK", "0") not in ("", "0") else ""))
                                     if kn.fork_branches() else "camera encoders x 2 only (HULC_FORK=0)",
                   "frames": "HBM-resident uint8 episode store, new play windows (20..32 steps, padded by repetition) every step, conv1 reads "
                             "the store through index rows" if args.episode_store
                             else "uint8 NHWC + RandomShiftsAug offsets, scaled/normalised while staging conv1" if args.uint8_frames
                             else "fp32 NCHW, already transformed (the reference's dataloader output)",
                   "gradient_allreduce": (f"{trainer.comm.algo} / {trainer.comm.payload} payload, backend {backend}"
                                          + (" (single rank, forced: exercises the collective path)" if world == 1 else ""))
                                         if dist.is_initialized() else "none (one rank, no process group)",
                   "exact_forward_sites": (",".join(sorted(kn.fp32_sites())) or "none") if args.compute == "bf16" and not args.affordance else None,
                   "final_loss": round(final_loss, 4)},
    }
    if rl is not None:
        # step_frac = the WHOLE step against the dense MFMA roof (the roof that bounds this path), on the algorithmic
        # 14.13 GFLOP / sequence; frac / achieved describe the single dominant kernel only
        kernel_ms = rl.pop("gpu_kernel_ms_per_step")
        out["roofline"] = {"step_frac": step_frac, **rl, "step_frac_of_mfma_peak": step_frac, "gpu_kernel_ms_per_step": kernel_ms}
    if rl_txl is not None:
        out["roofline_txl"] = rl_txl
    if comm_info is not None:
        out["comm"] = comm_info
    plain = not (args.real_world or args.uint8_frames or args.episode_store or args.no_graph or args.affordance)
    if args.full and world == 1 and args.compute == "bf16" and plain and not args.no_secondary:
        del trainer, model
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        out["secondary"] = secondary_mode(args, dev, "fp32")            # (key kept from round 2: the exact-fp32 leg)
        gc.collect()
        torch.cuda.empty_cache()
        out["secondary_mixed"] = secondary_mode(args, dev, "mixed")
        gc.collect()
        torch.cuda.empty_cache()
        out["secondary_exact_sites"] = secondary_mode(args, dev, "bf16+sites")
        gc.collect()
        torch.cuda.empty_cache()
        out["secondary_a3"] = secondary_mode(args, dev, "bf16+a3")
        gc.collect()
        torch.cuda.empty_cache()
        out["secondary_lightning_loop"] = lightning_loop(args, dev)
    if args.full and rank == 0 and not args.no_cpu_baseline and world == 1:
        out["cpu_baseline"] = cpu_baseline_affordance() if args.affordance else cpu_baseline()
    if rank == 0:
        emit(out)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
