"""Native training loop for the hot path: flat HBM arenas, fused Adam, RCCL gradient all-reduce.

The reference trains through pytorch-lightning (hulc2/training.py:64-82: Trainer.fit -> training_step ->
backward -> DDP bucketed all-reduce -> Adam step).  Lightning is a third-party layer outside the hot-path scope
(SURVEY.md §2 L3); this file is the MI355X-native equivalent of exactly that inner loop:

  * all trainable parameters live in ONE contiguous fp32 arena (params / grads / exp_avg / exp_avg_sq share
    offsets) plus a bf16 shadow arena the MFMA kernels read — 47 M params = 188 MB x4 + 94 MB of 288 GB HBM
  * the optimizer is one HBM-streaming kernel launch over the arena (hulc_adam_step) that also refreshes the
    bf16 shadow — torch.optim.Adam semantics (hulc2.py:185-198, lr 2e-4); `optimizer="adamw" | "sgd"` selects hulc_adamw_step /
    hulc_sgd_step, the other two configs of conf/model/optimizer/ (SGD: one state arena, or none without momentum)
  * data parallelism: gradient buckets are contiguous slices of the grad arena, all-reduced in place (no
    flatten/unflatten copies) on a side HIP stream as soon as autograd has produced every gradient of the
    bucket; the 1/world scale is folded into the Adam kernel.  One process per GPU, torch.distributed
    ("nccl" = RCCL over xGMI on ROCm; "gloo" in the CPU tests).
"""
from typing import Dict, List, Optional

import contextlib
import copy
import ctypes

import torch
import torch.distributed as dist

from . import gradsink
from . import kernels as kn
from . import shadow
from . import switches
from .arena import MAX_KERNEL_RANGES, WeightKeeper, plan_arena, span_ranges


class GradComm:
    """Sums slices of the fp32 gradient arena over the ranks, in place (replaces the NCCL ring inside Lightning's DDPStrategy,
    hulc2/training.py:72-75).

      algo     "ring"   one dist.all_reduce per slice (RCCL picks the algorithm; on xGMI a ring is bound by ONE of the 7 links)
               "direct" all_to_all_single -> local sum of the W contributions of this rank's chunk in rank order (hulc_sum_chunks, fp32
                        accumulation) -> all_gather_into_tensor: every rank talks to every peer at once, so all 7 links carry 1/W of the
                        payload each way; the result is bit-identical on all ranks (one rank reduces a chunk, everyone receives it)
      payload  "fp32"   the arena slice as it is
               "bf16"   rounded to bf16 for the wire (half the bytes), widened back into the arena afterwards; changes the arithmetic
                        (gradients pick up one bf16 rounding, the sum of "direct" a second one), hence a switch
    Defaults (HULC_ALLREDUCE / HULC_GRAD_PAYLOAD override them):
      payload  fp32 at every world size — the reference's DDP all-reduce is fp32 (hulc2/training.py:72-75), and the arithmetic of the
               gradients must not depend on how many ranks a job has.  bf16 is opt-in (HULC_GRAD_PAYLOAD=bf16 / grad_payload="bf16"): half the
               bytes for one bf16 rounding of the summands; with bf16 and algo "auto" the exchange is always "direct" (hulc_sum_chunks
               accumulates in fp32: one rounding) — "ring" with a bf16 buffer lets RCCL add in bf16 at every hop (W - 1 roundings) and runs
               only when asked for by name.
      algo     "auto" (fp32): on GPUs with world >= 2 both algorithms are TIMED once on the real fabric when the trainer is built (three
               reductions of a 32 MB slice each, max over ranks; the ranks agree on every step of the probe before they enter a collective)
               and the faster one is kept — whether RCCL's own multi-ring all-reduce or the direct exchange wins on an 8-GPU xGMI mesh is a
               property of the node.  Ring and direct sum in different orders, so the choice is part of a run's numerics: it is printed
               (bench.py's line, `describe()`), stored in ArenaTrainer.state_dict()["comm"], re-applied by load_state_dict, and pinned with
               HULC_ALLREDUCE=ring|direct.  On CPU (gloo) auto = ring."""

    def __init__(self, flat_grad: torch.Tensor, group=None, algo: Optional[str] = None, payload: Optional[str] = None, force: bool = False):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.active = self.world > 1 or (force and dist.is_initialized())
        self.algo = algo or switches.value("ALLREDUCE") or "auto"
        self.payload = payload or switches.value("GRAD_PAYLOAD") or self.default_payload(self.world)
        if self.algo not in ("ring", "direct", "auto") or self.payload not in ("fp32", "bf16"):
            raise ValueError(f"gradient all-reduce: algo {self.algo!r} (ring | direct | auto), payload {self.payload!r} (fp32 | bf16)")
        self.flat_grad = flat_grad
        self.on_gpu = flat_grad.is_cuda
        self._bufs = {}
        self.probe_ms: Dict[str, float] = {}
        self.chosen_by = "pinned"
        if self.algo == "auto":
            fabric = self.active and self.on_gpu and self.world > 1 and dist.get_backend(group) == "nccl"     # (gloo: host staging, nothing to tune)
            if self.payload == "bf16":
                self.algo, self.chosen_by = "direct", "rule (bf16 payload: fp32-accumulating exchange)"
            elif fabric:
                self.algo, self.chosen_by = self._probe(), "probe"
            else:
                self.algo, self.chosen_by = "ring", "rule (no fabric to probe)"

    @staticmethod
    def default_payload(world: int) -> str:
        return "fp32"

    def pin(self, algo: str) -> None:
        """re-apply a recorded choice (ArenaTrainer.load_state_dict): a resumed run keeps the summation order it started with"""
        if algo not in ("ring", "direct"):
            raise ValueError(f"gradient all-reduce: cannot pin {algo!r}")
        if algo != self.algo:
            self.algo, self.chosen_by = algo, "checkpoint"
            self._bufs = {}

    def _agree(self, ok: bool) -> bool:
        """True when EVERY rank says ok — a rank that failed locally (allocation) must not leave its peers alone inside a collective"""
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.flat_grad.device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=self.group)
        return bool(int(t.item()))

    PROBE_ELEMS = 8 << 20          # 32 MB of fp32 gradients: enough to be bandwidth-bound on xGMI, small next to the 288 GB

    def _probe(self) -> str:
        """time both algorithms on a bounded scratch slice (the gradients are not touched) and keep the faster; every rank sees the same
        max-over-ranks timings, so every rank makes the same choice.  Local failures (an allocation) are agreed on with an all_reduce(MIN)
        BEFORE the ranks enter the algorithm's collectives; the staging buffers of the probe are dropped afterwards."""
        keep = self.flat_grad
        n = min(keep.numel(), self.PROBE_ELEMS)
        scratch = None
        try:
            scratch = torch.zeros(n, dtype=keep.dtype, device=keep.device)
        except Exception as e:                                      # noqa: BLE001
            self.probe_error = f"scratch: {type(e).__name__}: {e}"
        if not self._agree(scratch is not None):
            return "ring"
        self.flat_grad = scratch
        try:
            for algo in ("ring", "direct"):
                self.algo = algo
                ok = True
                try:
                    self.reserve()                                  # local: staging buffers of this algorithm
                except Exception as e:                              # noqa: BLE001
                    ok, self.probe_error = False, f"{algo}: {type(e).__name__}: {e}"
                if not self._agree(ok):
                    self.probe_ms[algo] = float("inf")
                    continue
                self.reduce(0, n)                                   # warm-up: communicators (an error HERE is every rank's error: it propagates)
                if self.on_gpu:
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(3):
                        self.reduce(0, n)
                    e1.record()
                    torch.cuda.synchronize()
                    ms = e0.elapsed_time(e1) / 3
                else:                                               # (host process groups: the same probe on the wall clock — what the CPU tests run)
                    import time
                    t0 = time.perf_counter()
                    for _ in range(3):
                        self.reduce(0, n)
                    ms = (time.perf_counter() - t0) / 3 * 1e3
                t = torch.tensor([ms], dtype=torch.float32, device=keep.device)
                dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)      # (every rank sees the slowest rank's time)
                self.probe_ms[algo] = round(float(t.item()), 4)
        finally:
            self.flat_grad = keep
            self._bufs = {}                                         # (reserve() re-creates what the chosen algorithm needs, at arena size)
        best = min(self.probe_ms, key=self.probe_ms.get)
        return best if self.probe_ms[best] != float("inf") else "ring"

    def describe(self) -> Dict:
        """what bench.py prints about the gradient exchange: algorithm, payload, bytes, the probe's timings"""
        n = self.flat_grad.numel()
        payload_bytes = n * (2 if self.payload == "bf16" else 4)
        sent = int(2 * (self.world - 1) / max(self.world, 1) * payload_bytes)
        return {"algo": self.algo, "chosen_by": self.chosen_by, "payload": self.payload, "gradient_bytes": payload_bytes, "bytes_sent_per_rank_per_step": sent,
                "probe_ms": {k: (v if v != float("inf") else None) for k, v in self.probe_ms.items()},
                **({"probe_error": self.probe_error} if getattr(self, "probe_error", None) else {})}

    def _buf(self, name: str, n: int, dtype) -> torch.Tensor:
        t = self._bufs.get(name)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = self._bufs[name] = torch.zeros(max(n, self.flat_grad.numel() + 8 * self.world), dtype=dtype, device=self.flat_grad.device)
        return t[:n]

    def reserve(self) -> None:
        """allocate the staging buffers up front (before a hipGraph capture pins the allocator pools)"""
        if not self.active or (self.algo == "ring" and self.payload == "fp32"):
            return
        dt = torch.bfloat16 if self.payload == "bf16" else torch.float32
        self._buf("stage", 1, dt)
        if self.algo == "direct":
            self._buf("recv", 1, dt)
            self._buf("mine", 1, dt)

    def _narrow(self, src: torch.Tensor, dst: torch.Tensor) -> None:
        if self.on_gpu and dst.dtype == torch.bfloat16:
            kn.cast_f32_to_bf16(src, dst, src.numel())
        else:
            dst.copy_(src)

    def _widen(self, src: torch.Tensor, dst: torch.Tensor) -> None:
        if self.on_gpu and src.dtype == torch.bfloat16:
            kn.cast_bf16_to_f32(src, dst, src.numel())
        else:
            dst.copy_(src)

    def reduce(self, lo: int, hi: int, async_op: bool = False):
        """flat_grad[lo:hi] <- sum over ranks, on the current stream.  Returns a work handle only for async_op (CPU ring/fp32 path)."""
        view = self.flat_grad[lo:hi]
        n = hi - lo
        if n <= 0 or not self.active:
            return None
        if self.algo == "ring" and self.payload == "fp32":
            return dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=async_op)
        dt = torch.bfloat16 if self.payload == "bf16" else torch.float32
        if self.algo == "ring":
            stage = self._buf("stage", n, dt)
            self._narrow(view, stage)
            dist.all_reduce(stage, op=dist.ReduceOp.SUM, group=self.group)
            self._widen(stage, view)
            return None
        W = self.world
        chunk = ((n + W - 1) // W + 7) // 8 * 8
        stage, recv, mine = self._buf("stage", chunk * W, dt), self._buf("recv", chunk * W, dt), self._buf("mine", chunk, dt)
        self._narrow(view, stage[:n])
        if chunk * W > n:
            stage[n:].zero_()
        dist.all_to_all_single(recv, stage, group=self.group)
        if self.on_gpu:
            kn.sum_chunks(recv, W, chunk, mine)
        else:
            mine.copy_(recv.view(W, chunk).float().sum(0))
        dist.all_gather_into_tensor(stage, mine, group=self.group)
        self._widen(stage[:n], view)
        return None


class GradBuckets:
    """Contiguous slices of the gradient arena reduced across ranks, overlapped with backward."""

    def __init__(self, params: List[torch.nn.Parameter], offsets: List[int], flat_grad: torch.Tensor, bucket_bytes: int,
                 group=None, overlap: bool = True, comm: Optional[GradComm] = None):
        self.group = group
        self.comm = comm if comm is not None else GradComm(flat_grad, group)
        self.world = self.comm.world
        self.active = self.comm.active
        self.flat_grad = flat_grad
        self.on_gpu = flat_grad.is_cuda
        self.comm_stream = torch.cuda.Stream() if self.on_gpu else None
        # autograd finishes parameters roughly in reverse registration order: build buckets from the arena's tail
        self.buckets: List[Dict] = []
        cur = {"lo": None, "hi": None, "n": 0, "pending": 0}
        cap = max(bucket_bytes // 4, 1)
        self.param_bucket: Dict[int, int] = {}
        for p, off in reversed(list(zip(params, offsets))):
            n = p.numel()
            if cur["n"] and cur["n"] + n > cap:
                self.buckets.append(cur)
                cur = {"lo": None, "hi": None, "n": 0, "pending": 0}
            cur["lo"] = off
            cur["hi"] = cur["hi"] if cur["hi"] is not None else off + n
            cur["n"] += n
            self.param_bucket[id(p)] = len(self.buckets)
        if cur["n"]:
            self.buckets.append(cur)
        self.members = [0] * len(self.buckets)
        for b in self.param_bucket.values():
            self.members[b] += 1
        self.handles = []
        self.overlap = overlap
        self._hook_handles = []
        if self.active and overlap:
            for p in params:
                self._hook_handles.append(p.register_post_accumulate_grad_hook(self._hook))
        self.reset()

    def close(self) -> None:
        """remove the per-parameter hooks (a dead trainer's buckets must not keep launching all-reduces on its arena)"""
        for h in self._hook_handles:
            h.remove()
        self._hook_handles = []

    def reset(self):
        for i, b in enumerate(self.buckets):
            b["pending"] = self.members[i]
        self.handles = []

    def _launch(self, b):
        if self.on_gpu:
            self.comm_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.comm_stream):
                self.comm.reduce(b["lo"], b["hi"])
        else:
            h = self.comm.reduce(b["lo"], b["hi"], async_op=True)
            if h is not None:
                self.handles.append(h)

    def _hook(self, p):
        b = self.buckets[self.param_bucket[id(p)]]
        b["pending"] -= 1
        if b["pending"] == 0:
            self._launch(b)

    def finish(self):
        """Flush buckets whose parameters produced no gradient this step, then join the comm stream."""
        if self.active and not self.overlap:       # graph mode, eager step: one in-place all-reduce of the whole arena
            # Always on the comm stream, never on the caller's: ProcessGroupNCCL records the work's end event on the stream the collective
            # runs on, and its watchdog thread keeps querying that event for a while after the work is done.  capture() runs its warm-up
            # steps on the very stream it captures next — an event of that stream queried during capture is hipErrorCapturedEvent and the
            # watchdog aborts the process (found by the first RCCL run on hardware, round 2).
            if self.on_gpu:
                cur = torch.cuda.current_stream()
                self.comm_stream.wait_stream(cur)
                with torch.cuda.stream(self.comm_stream):
                    self.comm.reduce(0, self.flat_grad.numel())
                cur.wait_stream(self.comm_stream)
            else:
                self.comm.reduce(0, self.flat_grad.numel())
            return
        if self.active:
            for b in self.buckets:
                if b["pending"] > 0:
                    b["pending"] = 0
                    self._launch(b)
            for h in self.handles:
                h.wait()
            if self.on_gpu:
                torch.cuda.current_stream().wait_stream(self.comm_stream)
        self.reset()


class ArenaTrainer(WeightKeeper):
    """The native loop on the weight keeper's arenas: the gradient arena, the arena optimizer (moments, three update rules, the lr schedule,
    the state dicts), the gradient exchange (GradComm / GradBuckets) and step() / capture() / replay()."""

    def __init__(self, model: torch.nn.Module, lr: float = 2e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 bucket_mb: int = 32, group=None, overlap: bool = True, comm_algo: Optional[str] = None, grad_payload: Optional[str] = None,
                 force_comm: bool = False, optimizer: str = "adam", momentum: float = 0.0, dampening: float = 0.0, nesterov: bool = False,
                 skip_params=(), gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: str = "norm",
                 accumulate_grad_batches: int = 1):
        """optimizer: the update rule of optimizer_step() — "adam" (torch.optim.Adam, L2 weight decay), "adamw" (torch.optim.AdamW, decoupled
        decay) or "sgd" (torch.optim.SGD with momentum / dampening / nesterov, L2 weight decay): conf/model/optimizer/{adam,adamw,sgd}.yaml;
        hulc2_amd.optim.trainer_kwargs_from_config maps such a config to these arguments.
        skip_params (adamw / sgd): parameters that never receive a gradient.  Their arena ranges (neighbours merged, at most 8) are left
        untouched by the step, as torch leaves a parameter without a gradient — weight decay would shrink them otherwise.
        gradient_clip_val / gradient_clip_algorithm: Lightning's trainer flags of the same names (0 / None: off).  "norm": the global L2 norm
        of the finished (all-reduced, 1 / world scaled) gradient arena is taken by one deterministic pass (hulc_grad_norm_clip) and the
        step multiplies every gradient by min(1, gradient_clip_val / (norm + 1e-6)) in registers, as torch.nn.utils.clip_grad_norm_ would
        have in memory; "value": the step clamps every gradient to [-gradient_clip_val, gradient_clip_val] (clip_grad_value_).  Every rank
        reads the same arena with the same kernel, so all ranks apply the same bits; set_gradient_clip changes the threshold later.
        accumulate_grad_batches: Lightning's trainer flag of the same name, k >= 1.  Every step() / replay() is one micro-batch and returns its
        detached loss; calls are grouped into windows of k and the optimizer runs once per window, on G = ((g_1 + g_2) + ... + g_k) * s with
        s = fp32(1 / k) (the quotient formed in double, then rounded), summed left to right in fp32 by hulc_grad_accumulate into a second
        gradient arena (flat_acc).  That is Lightning's mean over the window up to rounding: Lightning divides each LOSS by k, here the SUM is
        scaled once.  A micro-batch that does not close its window runs forward, backward and one accumulate launch, nothing else: no
        exchange, lr write, norm pass, optimizer launch or derive_after_step.  The closing one runs today's tail on G — the gradient
        exchange (ONCE per window: under data parallelism the collectives drop k-fold, which is the point of accumulating there), the lr
        schedule, clipping (grad_norm is the norm of G), the optimizer, the derived copies.  The optimizer step count (host and device) and
        the lr schedule advance once per window, the RNG word once per micro-batch (fresh dropout masks and plan samples).  With several
        ranks k > 1 needs overlap=False: the bucket hooks would reduce every micro-batch's partial gradient.  k == 1 allocates no
        accumulator and runs exactly the launches it always ran.
        force_comm: run the multi-rank control flow (split graphs, comm stream, collectives) even with a single rank in the process
        group — how the RCCL path is exercised on a one-GPU box."""
        if optimizer not in ("adam", "adamw", "sgd"):
            raise ValueError(f"ArenaTrainer: optimizer {optimizer!r} is not one of 'adam', 'adamw', 'sgd'")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")          # (torch.optim.SGD's own refusal)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.optimizer, self.momentum, self.dampening, self.nesterov = optimizer, float(momentum), float(dampening), bool(nesterov)
        self.base_lr = lr                                  # what a schedule's factor multiplies (torch: the group's initial_lr)
        self.clip_val, self.clip_algorithm = self._check_clip(gradient_clip_val, gradient_clip_algorithm)
        self.step_node = False                             # (the step node is the keeper's, under an external optimizer)
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.multi = self.world > 1 or (force_comm and dist.is_initialized())
        self.accumulate_grad_batches = self._check_accumulate(accumulate_grad_batches, self.multi and overlap)
        # fused views receive their gradient through a sink only, so they exist only when sinks do (not with per-parameter all-reduce hooks)
        use_sinks = next(p for p in model.parameters() if p.requires_grad).is_cuda and (not self.multi or not overlap)
        plan = plan_arena(model, use_sinks)
        self.skip_ranges = self._skip_ranges(plan, skip_params)
        self._install(model, plan, grad_arena=True)
        dev, total = self.dev, self.total
        for p, off in zip(self.params, self.offsets):
            p.grad = self.flat_g[off:off + p.numel()].view(p.shape)
        # SGD: exp_avg serves as the momentum buffer (none with momentum == 0), there is no second state arena
        sgd = self.optimizer == "sgd"
        self.exp_avg = torch.zeros(0 if sgd and self.momentum == 0 else total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(0 if sgd else total, dtype=torch.float32, device=dev)
        self.comm = GradComm(self.flat_g, group, comm_algo, grad_payload, force=force_comm)
        self.buckets = GradBuckets(self.params, self.offsets, self.flat_g, bucket_mb << 20, group, overlap, comm=self.comm)
        # bucket all-reduces overlapped with backward share the GPU with the compute stream: barrier kernels are then off
        kn.set_concurrent_streams(dev.type == "cuda" and self.multi and overlap)
        self._acc_hooks = []
        if use_sinks:                                      # no per-parameter all-reduce hooks depend on AccumulateGrad
            self._register_sinks(None)
            self._acc_hooks = [p.register_post_accumulate_grad_hook(self._saw_autograd_grad) for p in self.params]
        self._clip_out = torch.zeros(2, dtype=torch.float32, device=dev)      # {gradient norm, clip coefficient} of the last norm pass
        self.micro_batch = 0                               # position inside the current accumulation window, 0 .. k - 1
        self.flat_acc = self._new_accumulator()            # the running sum of a window's gradients (None with k == 1)
        self.step_count = 0
        self._fault_every = switches.value("FAULT_CHECK_EVERY")
        if dev.type == "cuda":
            kn.step_state(dev)[1] = 0               # the device-resident Adam step count starts with this trainer (the RNG word keeps walking)
        self.graph_fb = self.graph_enc = self.graph_opt = None
        self.static_loss = None
        self._comm_events = []
        self._split_encoder(model)

    def _split_encoder(self, model) -> None:
        """Split point for overlapping the gradient all-reduce with the tail of backward in graph mode: the camera encoders are registered
        first (arena head, 0.75 M parameters) but their backward (the conv stack) is the LAST ~2 ms of a step, while everything else (98 % of
        the gradient bytes) is complete once backward reaches the encoder output."""
        names = {id(p): n for n, p in model.named_parameters()}
        enc = [names.get(id(p), "").startswith("perceptual_encoder.") for p in self.params]
        idx = [i for i, e in enumerate(enc) if e]
        self.enc_lo = self.enc_hi = 0                      # arena slice [enc_lo, enc_hi) = the encoder gradients (one contiguous run)
        self.enc_params, self.rest_params = [], list(self.params)
        if idx and len(idx) < len(self.params) and idx[-1] - idx[0] + 1 == len(idx) and hasattr(model, "perceptual_encoder"):
            (self.enc_lo, self.enc_hi), = self.span_ranges(idx)
            self.enc_params = [self.params[i] for i in idx]
            self.rest_params = [p for i, p in enumerate(self.params) if not enc[i]]
            model.perceptual_encoder.register_forward_hook(self._keep_encoder_output)
        self._emb = None

    def _skip_ranges(self, plan, skip_params) -> list:
        """arena ranges of the parameters the optimizer pass leaves alone (arena.span_ranges), checked against what the kernels take"""
        skip = {id(p) for p in skip_params}
        if not skip:
            return []
        if self.optimizer == "adam":
            raise ValueError("ArenaTrainer: skip_params needs optimizer='adamw' or 'sgd' (the Adam pass has no skip ranges)")
        unknown = skip - {id(p) for p in plan.params}
        if unknown:
            raise ValueError(f"ArenaTrainer: {len(unknown)} of skip_params are not trainable parameters of the model")
        ranges = span_ranges(plan.offsets, plan.total, [i for i, p in enumerate(plan.params) if id(p) in skip])
        if len(ranges) > MAX_KERNEL_RANGES:
            raise ValueError(f"ArenaTrainer: skip_params make {len(ranges)} arena ranges, the optimizer kernels take at most {MAX_KERNEL_RANGES}")
        if any(a % 4 for a, _ in ranges):
            raise ValueError("ArenaTrainer: a skipped parameter sits at an arena offset that is no multiple of 4 (member of a fused group)")
        return ranges

    def __deepcopy__(self, memo):
        """a trainer copies like any object (only a model's own keeper stays behind when the model is copied)"""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__dict__.update(copy.deepcopy(self.__dict__, memo))
        return new

    # ---- optimizer state ---------------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict:
        """optimizer state in the reference's terms (a Lightning checkpoint carries torch.optim.Adam's exp_avg / exp_avg_sq / step per
        parameter, hulc2.py:185-198): per-parameter tensors keyed by the model's parameter names, so the arena layout can change between
        save and load; plus the device step words (Adam step count, RNG word)."""
        names = {id(p): n for n, p in self.model.named_parameters()}
        st = {}
        for p, off in zip(self.params, self.offsets):
            n = p.numel()
            if self.optimizer == "sgd":                           # torch.optim.SGD's record; nothing without momentum
                st[names[id(p)]] = {"momentum_buffer": self.exp_avg[off:off + n].view(p.shape).clone()} if self.momentum != 0 else {}
                continue
            st[names[id(p)]] = {"exp_avg": self.exp_avg[off:off + n].view(p.shape).clone(),
                                "exp_avg_sq": self.exp_avg_sq[off:off + n].view(p.shape).clone()}
        words = kn.step_state(self.dev).tolist() if self.dev.type == "cuda" else [0, self.step_count]
        # the accumulation window: its length and the position inside it; an open window (position > 0) carries its running sum the way the
        # moments travel, per parameter and by name.  (The device step count of an open window already counts the step that will close it.)
        acc = {"k": int(self.accumulate_grad_batches), "position": int(self.micro_batch)}
        if self.micro_batch > 0:
            acc["sum"] = {names[id(p)]: self.flat_acc[off:off + p.numel()].view(p.shape).clone() for p, off in zip(self.params, self.offsets)}
        # (the schedule's function is not state, as with torch's LambdaLR: the resumed run attaches the same one, before or after loading)
        return {"lr_schedule": {"base_lr": float(self.base_lr), "position": int(self._opt_steps), "device_lr": self._lr_dev is not None},
                "state": st, "accumulate": acc, "step": int(self.step_count), "rng_word": int(words[0]), "device_step": int(words[1]),
                "comm": ({"algo": self.comm.algo, "payload": self.comm.payload, "chosen_by": self.comm.chosen_by} if self.comm is not None else None),
                "hparams": {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd, "optimizer": self.optimizer,
                            "momentum": self.momentum, "dampening": self.dampening, "nesterov": self.nesterov}}

    def load_state_dict(self, sd: Dict) -> None:
        kind = sd.get("hparams", {}).get("optimizer", "adam")     # (states written before there was a choice are Adam's)
        if kind != self.optimizer:
            raise ValueError(f"ArenaTrainer.load_state_dict: the state is of optimizer {kind!r}, this trainer was built with "
                             f"optimizer={self.optimizer!r}; build the trainer with the optimizer the state was saved under")
        acc = sd.get("accumulate") or {"k": self.accumulate_grad_batches, "position": 0}      # (states written before there were windows)
        if int(acc["k"]) != self.accumulate_grad_batches:
            raise ValueError(f"ArenaTrainer.load_state_dict: the state was saved with accumulate_grad_batches={int(acc['k'])}, this trainer "
                             f"was built with {self.accumulate_grad_batches}; build the trainer with the window length of the state")
        names = {n: p for n, p in self.model.named_parameters()}
        index = {id(p): off for p, off in zip(self.params, self.offsets)}
        missing = [n for n, p in names.items() if id(p) in index and n not in sd["state"]]
        if missing:
            raise KeyError(f"ArenaTrainer.load_state_dict: no optimizer state for {missing[:4]}{'...' if len(missing) > 4 else ''}")
        position = int(acc["position"])
        if not 0 <= position < self.accumulate_grad_batches:
            raise ValueError(f"ArenaTrainer.load_state_dict: window position {position} outside 0 .. {self.accumulate_grad_batches - 1}")
        if position > 0:
            lost = [n for n, p in names.items() if id(p) in index and n not in acc.get("sum", {})]
            if lost:
                raise KeyError(f"ArenaTrainer.load_state_dict: no accumulated gradient for {lost[:4]}{'...' if len(lost) > 4 else ''}")
            with torch.no_grad():
                self.flat_acc.zero_()
                for n, t in acc["sum"].items():
                    p = names.get(n)
                    if p is not None and id(p) in index:
                        self.flat_acc[index[id(p)]:index[id(p)] + p.numel()].copy_(t.reshape(-1))
        self.micro_batch = position
        with torch.no_grad():
            for n, rec in sd["state"].items():
                p = names.get(n)
                if p is None or id(p) not in index:
                    continue
                off, k = index[id(p)], p.numel()
                if self.optimizer == "sgd":
                    if self.exp_avg.numel():
                        self.exp_avg[off:off + k].copy_(rec["momentum_buffer"].reshape(-1))
                    continue
                self.exp_avg[off:off + k].copy_(rec["exp_avg"].reshape(-1))
                self.exp_avg_sq[off:off + k].copy_(rec["exp_avg_sq"].reshape(-1))
        self.step_count = int(sd["step"])
        hp = sd.get("hparams", {})
        if self.optimizer == "sgd" and (float(hp.get("momentum", self.momentum)) != 0) != (self.exp_avg.numel() != 0):
            raise ValueError("ArenaTrainer.load_state_dict: the state and this trainer disagree on whether SGD keeps a momentum buffer")
        sched = sd.get("lr_schedule")
        if sched is not None:                                     # the resumed run continues the same learning-rate sequence
            self.base_lr, self._opt_steps = float(sched["base_lr"]), int(sched["position"])
            if sched.get("device_lr") and self._lr_dev is None:
                self.set_lr(hp.get("lr", self.lr))
        self._set_hparams(hp.get("lr", self.lr), hp.get("betas", self.betas), hp.get("eps", self.eps), hp.get("weight_decay", self.wd),
                          momentum=hp.get("momentum", self.momentum), dampening=hp.get("dampening", self.dampening),
                          nesterov=hp.get("nesterov", self.nesterov))
        algo = (sd.get("comm") or {}).get("algo")
        if algo in ("ring", "direct") and self.comm is not None and self.comm.active and not switches.value("ALLREDUCE"):
            self.comm.pin(algo)                                   # a resumed run keeps the summation order it started with
        if self.dev.type == "cuda":
            kn.reset_step_state(self.dev, seed=int(sd["rng_word"]), step=int(sd.get("device_step", sd["step"])))
        self.refresh_shadows()

    # ---- interchange with the reference's checkpoints: `optimizer_states[0]` of a Lightning checkpoint IS torch.optim.Adam.state_dict() ----------
    def _torch_state_names(self) -> tuple:
        """the per-parameter state tensors of the torch optimizer of this trainer's kind, in the order (exp_avg, exp_avg_sq) of the arenas"""
        if self.optimizer == "sgd":
            return ("momentum_buffer",) if self.exp_avg.numel() else ()
        return ("exp_avg", "exp_avg_sq")

    def to_torch_optimizer_state_dict(self) -> Dict:
        """This trainer's state as the `state_dict()` of the torch optimizer of its kind holds it (torch 2.10; reference: hulc2.py:185-198,
        conf/model/optimizer/*.yaml): `state` keyed by the INDEX of the parameter in `model.parameters()` order, `param_groups[0]["params"]`
        = all indices.  torch.optim.Adam / AdamW keep `step` / `exp_avg` / `exp_avg_sq` per parameter and differ in `decoupled_weight_decay`;
        torch.optim.SGD's state is `momentum_buffer` alone (no entry without momentum).  Frozen / never-updated parameters and skip_params
        have no entry: torch never made state for them.  A reference Lightning run resumes from it with `optimizer.load_state_dict(...)`."""
        order = list(self.model.parameters())
        index = {id(p): off for p, off in zip(self.params, self.offsets)}
        skipped = lambda off: any(a <= off < b for a, b in self.skip_ranges)
        sgd, names = self.optimizer == "sgd", self._torch_state_names()
        state = {}
        if self.step_count > 0 and names:
            for i, p in enumerate(order):
                off = index.get(id(p))
                if off is None or skipped(off):
                    continue
                state[i] = {} if sgd else {"step": torch.tensor(float(self.step_count))}
                for name, arena in zip(names, (self.exp_avg, self.exp_avg_sq)):
                    state[i][name] = arena[off:off + p.numel()].view(p.shape).clone()
        lr = self.lr
        if self._lr_lambda is not None:                           # what a torch scheduler leaves behind k steps: base * lambda(k) and initial_lr
            lr = float(self.base_lr) * self._lr_lambda(self._opt_steps)
        if sgd:
            group = {"lr": lr, "momentum": self.momentum, "dampening": self.dampening, "weight_decay": self.wd, "nesterov": self.nesterov,
                     "maximize": False, "foreach": None, "differentiable": False, "fused": None}
        else:
            group = {"lr": lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd, "amsgrad": False, "maximize": False,
                     "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                     "decoupled_weight_decay": self.optimizer == "adamw"}
        group["params"] = list(range(len(order)))
        if self._lr_lambda is not None:
            group["initial_lr"] = float(self.base_lr)
        return {"state": state, "param_groups": [group]}

    def from_torch_optimizer_state_dict(self, sd: Dict) -> None:
        """Resume from the `state_dict()` of the torch optimizer of this trainer's kind (a reference checkpoint's `ckpt["optimizer_states"][0]`):
        the inverse of to_torch_optimizer_state_dict.  An AdamW trainer refuses a group without decoupled decay (that is torch.optim.Adam's
        rule: optimizer="adam"), and the other way round.  The fused kernels keep ONE step count, so the per-parameter steps must agree (they
        do for an optimizer that stepped all its parameters together).  torch.optim.SGD keeps no step count: a state WITH momentum buffers
        resumes behind the first step, one without starts at it.  Adam's form may come in several param_groups (their ids are flattened, the
        hyper-parameters are group 0's)."""
        groups = sd["param_groups"]
        g0 = groups[0]
        sgd, adam = self.optimizer == "sgd", self.optimizer == "adam"
        if adam and g0.get("decoupled_weight_decay"):
            raise ValueError("the optimizer state decays decoupled (torch.optim.AdamW): build the trainer with optimizer='adamw'")
        if not adam and (sgd != ("momentum" in g0) or (not sgd and not g0.get("decoupled_weight_decay"))):
            raise ValueError(f"the optimizer state is not torch's for optimizer={self.optimizer!r} (group keys {sorted(k for k in g0 if k != 'params')})")
        if g0.get("amsgrad") or g0.get("maximize"):
            raise NotImplementedError("amsgrad / maximize are not built (conf/model/optimizer/*.yaml use neither)")
        if not adam and len(groups) != 1:
            raise NotImplementedError("several param groups are not built: the arena optimizer keeps one set of hyper-parameters")
        order = list(self.model.parameters())
        ids = [i for g in groups for i in g["params"]]
        if len(ids) != len(order):
            raise KeyError(f"optimizer state for {len(ids)} parameters, model.parameters() has {len(order)}")
        if sgd and (float(g0["momentum"]) != 0) != (self.exp_avg.numel() != 0):
            raise ValueError("the optimizer state and this trainer disagree on whether SGD keeps a momentum buffer")
        index = {id(p): off for p, off in zip(self.params, self.offsets)}
        names, steps = self._torch_state_names(), set()
        with torch.no_grad():
            for pos, key in enumerate(ids):
                p, rec = order[pos], sd["state"].get(key)
                off = index.get(id(p))
                if off is None:
                    continue
                if rec is not None and names and rec.get(names[0]) is None:
                    rec = None                                    # (no record: torch creates state lazily, a parameter that never saw a gradient)
                for name, arena in zip(names, (self.exp_avg, self.exp_avg_sq)):
                    if rec is None:
                        arena[off:off + p.numel()].zero_()
                        continue
                    if tuple(rec[name].shape) != tuple(p.shape):
                        raise KeyError(f"optimizer state {key}: shape {tuple(rec[name].shape)} vs parameter {tuple(p.shape)}")
                    arena[off:off + p.numel()].copy_(rec[name].reshape(-1))
                if rec is not None and names:
                    steps.add(1 if sgd else int(float(rec["step"])))
        if len(steps) > 1:
            raise ValueError(f"per-parameter steps differ ({sorted(steps)}): the arena optimizer keeps one step count")
        self.step_count = steps.pop() if steps else 0
        self._opt_steps = self.step_count                         # (a scheduler stepped once per optimizer step stands at the same count)
        if "initial_lr" in g0:
            self.base_lr = float(g0["initial_lr"])
        if sgd:
            self._set_hparams(g0["lr"], self.betas, self.eps, g0.get("weight_decay", 0.0), momentum=g0["momentum"],
                              dampening=g0.get("dampening", 0.0), nesterov=g0.get("nesterov", False))
        else:
            self._set_hparams(g0["lr"], g0["betas"], g0["eps"], g0.get("weight_decay", 0.0))
        if self.dev.type == "cuda":
            kn.step_state(self.dev)[1] = self.step_count
        self.refresh_shadows()

    def to_torch_adam_state_dict(self) -> Dict:
        """to_torch_optimizer_state_dict() of an Adam trainer: what `torch.optim.Adam(model.parameters(), lr).state_dict()` would hold"""
        if self.optimizer != "adam":
            raise ValueError(f"to_torch_adam_state_dict: this trainer's optimizer is {self.optimizer!r}; use to_torch_optimizer_state_dict()")
        return self.to_torch_optimizer_state_dict()

    def from_torch_adam_state_dict(self, sd: Dict) -> None:
        """from_torch_optimizer_state_dict() of an Adam trainer: resume from a reference checkpoint's `ckpt["optimizer_states"][0]`"""
        if self.optimizer != "adam":
            raise ValueError(f"from_torch_adam_state_dict: this trainer's optimizer is {self.optimizer!r}; use from_torch_optimizer_state_dict()")
        self.from_torch_optimizer_state_dict(sd)

    def _set_hparams(self, lr, betas, eps, wd, momentum=None, dampening=None, nesterov=None) -> None:
        """lr / betas / eps / weight decay are scalar kernel arguments: a captured optimizer graph has the OLD ones baked in, so a change
        after capture() drops the graphs — replay() then asks for a new capture() instead of silently stepping with the pre-load values
        (the lr in a Lightning checkpoint is the scheduler's current value, not the constructor's)."""
        momentum = self.momentum if momentum is None else float(momentum)
        dampening = self.dampening if dampening is None else float(dampening)
        nesterov = self.nesterov if nesterov is None else bool(nesterov)
        if (momentum != 0) != (self.momentum != 0) and self.optimizer == "sgd":
            raise ValueError("ArenaTrainer: SGD's momentum buffer is allocated (or not) at construction: momentum cannot change to or from 0")
        new = (float(lr), tuple(float(b) for b in betas), float(eps), float(wd), momentum, dampening, nesterov)
        old = (float(self.lr), tuple(float(b) for b in self.betas), float(self.eps), float(self.wd), self.momentum, self.dampening, self.nesterov)
        if self._lr_dev is not None:                              # device-lr mode (set_lr): the learning rate is no kernel argument
            self.set_lr(lr)
            new, old = new[1:], old[1:]
        self.lr, self.betas, self.eps, self.wd = lr, tuple(betas), eps, wd
        self.momentum, self.dampening, self.nesterov = momentum, dampening, nesterov
        if new != old and getattr(self, "graph_opt", None) is not None:
            self.graph_fb = self.graph_enc = self.graph_opt = None

    # ---- learning-rate schedules: the learning rate as a device scalar the captured optimizer launch reads --------------------------------
    _lr_dev = None                 # one fp32 element on the arena's device once set_lr() was called (device-lr mode); None = scalar kernel argument
    _lr_lambda = None              # the attached schedule (set_lr_schedule)
    _opt_steps = 0                 # optimizer steps this trainer has RUN (eager or replayed; a capture runs none): the schedule position

    def set_lr(self, lr: float) -> None:
        """The learning rate of the following optimizer steps, written into a device scalar the Adam kernel reads (hulc_adam_step_sched): a
        stream-ordered one-element fill, no host synchronisation, and captured graphs follow it.  The first call switches the trainer to this
        mode and drops graphs captured with the learning rate as a kernel argument (as _set_hparams does); later calls never drop one."""
        if self._lr_dev is None:
            self._lr_dev = torch.zeros(1, dtype=torch.float32, device=self.dev)
            if getattr(self, "graph_opt", None) is not None:
                self.graph_fb = self.graph_enc = self.graph_opt = None
        self._lr_dev.fill_(ctypes.c_float(lr).value)              # (rounded as the scalar kernel argument would be)
        self.lr = lr

    def set_lr_schedule(self, lr_lambda, base_lr: Optional[float] = None) -> None:
        """torch.optim.lr_scheduler.LambdaLR's contract (reference: hulc2/models/hulc2.py:185-198, `interval: step`): the trainer's k-th
        optimizer step, k from 0 and the warm-up steps of capture() included, runs with base_lr * lr_lambda(k), the product formed in Python
        floats.  step() and replay() write it in front of the optimizer launch / graph.  base_lr: default the trainer's current base."""
        if base_lr is not None:
            self.base_lr = float(base_lr)
        self._lr_lambda = lr_lambda
        self._apply_lr_schedule()

    def _apply_lr_schedule(self) -> None:
        if self._lr_lambda is not None:
            self.set_lr(float(self.base_lr) * self._lr_lambda(self._opt_steps))

    # ---- gradient clipping (Lightning: trainer.gradient_clip_val / gradient_clip_algorithm) ------------------------------------------------
    @staticmethod
    def _check_clip(val, algorithm):
        if algorithm not in ("norm", "value"):
            raise ValueError(f"ArenaTrainer: gradient_clip_algorithm {algorithm!r} is not 'norm' or 'value'")
        val = 0.0 if val is None else float(val)
        if not (0.0 <= val < float("inf")):
            raise ValueError(f"ArenaTrainer: gradient_clip_val must be finite and >= 0 (0 / None: off), got {val!r}")
        return val, algorithm

    def set_gradient_clip(self, val: Optional[float], algorithm: Optional[str] = None) -> None:
        """The clipping threshold (and, optionally, the algorithm) of the following optimizer steps; 0 / None switches clipping off.  Both are
        kernel arguments of the captured optimizer graph, so a change drops the graphs (as _set_hparams does for lr / betas): replay() then
        asks for a new capture() instead of clipping at the old threshold."""
        new = self._check_clip(val, self.clip_algorithm if algorithm is None else algorithm)
        if new != (self.clip_val, self.clip_algorithm) and getattr(self, "graph_opt", None) is not None:
            self.graph_fb = self.graph_enc = self.graph_opt = None
        self.clip_val, self.clip_algorithm = new

    @property
    def grad_norm(self) -> torch.Tensor:
        """one-element device tensor: the global L2 norm of the gradients the last optimizer step saw (before clipping), written by the norm
        pass of gradient_clip_algorithm="norm" — for logging without a synchronisation; it follows the replays of a captured graph."""
        return self._clip_out[0:1]

    def last_grad_norm(self) -> float:
        """grad_norm as a Python float.  SYNCHRONISES the host with the device (a .item()): call it where a sync happens anyway."""
        return float(self._clip_out[0].item())

    def _clip_args(self) -> dict:
        """launch the norm pass when clipping by norm and hand the step kernel its clipping arguments"""
        if not self.clip_val:
            return {}
        if self.clip_algorithm == "value":
            return {"clip_value": self.clip_val}
        kn.grad_norm_clip(self.flat_g, self.total, 1.0 / self.world, None, self.clip_val, self._clip_out)
        return {"clip_coef_dev": self._clip_out[1:2]}

    # ---- gradient accumulation (Lightning: trainer.accumulate_grad_batches) ----------------------------------------------------------------
    _replay_settle = ()            # arena slices the settle clean-up cleared behind the captured backward: replay() clears them again (k > 1)

    @staticmethod
    def _check_accumulate(k, hooks: bool = False) -> int:
        """hooks: the trainer reduces gradient buckets from per-parameter hooks (several ranks, overlap=True)"""
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"ArenaTrainer: accumulate_grad_batches must be an int >= 1, got {k!r}")
        if k > 1 and hooks:
            raise ValueError("ArenaTrainer: accumulate_grad_batches > 1 with several ranks needs overlap=False (the bucket hooks of "
                             "overlap=True would all-reduce every micro-batch's partial gradient)")
        return k

    def _new_accumulator(self) -> Optional[torch.Tensor]:
        if self.accumulate_grad_batches == 1:
            return None
        return torch.zeros(self.total, dtype=torch.float32, device=self.dev)

    def set_accumulate_grad_batches(self, k: int) -> None:
        """The window length of the following micro-batches; only at a window boundary (micro_batch == 0).  The captured graphs are built
        for one k (which launches they hold, who bumps the step count), so a change drops them, as set_gradient_clip does."""
        k = self._check_accumulate(k, self.multi and self.buckets.overlap)
        if self.micro_batch != 0:
            raise RuntimeError(f"ArenaTrainer.set_accumulate_grad_batches: micro-batch {self.micro_batch} of {self.accumulate_grad_batches} "
                               "is open; change the window length at a window boundary")
        if k == self.accumulate_grad_batches:
            return
        if getattr(self, "graph_opt", None) is not None:
            self.graph_fb = self.graph_enc = self.graph_opt = None
        self.accumulate_grad_batches = k
        self.flat_acc = self._new_accumulator()

    def _accumulate(self) -> bool:
        """behind the backward pass (and the settle clean-up) of a micro-batch, k > 1: the arena into the running sum — store, add, or finish
        back into flat_g.  True when this micro-batch closed its window (flat_g then holds G)."""
        j, k = self.micro_batch, self.accumulate_grad_batches
        if j == k - 1:
            kn.grad_accumulate(self.flat_acc, self.flat_g, self.total, "finish", ctypes.c_float(1.0 / k).value)
        else:
            kn.grad_accumulate(self.flat_acc, self.flat_g, self.total, "store" if j == 0 else "add")
        self.micro_batch = (j + 1) % k
        return j == k - 1

    # ---- KL annealing: the KL weight as a device scalar the captured KL launches read (Hulc2.set_kl_beta) --------------------------------
    _reg_captured = None           # Hulc2.regulariser_key() of the captured graphs (dropout probabilities, l2 flags)
    _kl_captured = None            # the by-value KL weight baked into the captured graphs; None: no graphs, or they read the model's device word
    _kl_schedule = None            # the attached annealing rule (set_kl_schedule)

    def set_kl_beta(self, beta: float) -> None:
        """The KL weight of the following steps (reference: hulc2/utils/kl_callbacks.py -> pl_module.set_kl_beta every epoch).  Forwards to the
        model, which on a GPU writes a device scalar the KL kernels read — a stream-ordered one-element fill, no host synchronisation, and
        captured graphs follow it.  The call that switches the model to that mode drops graphs captured with the weight as a kernel
        argument (as set_lr does for the learning rate); later calls never drop one."""
        self.model.set_kl_beta(beta)
        if self._kl_captured is not None and getattr(self.model, "kl_beta_on_device", False):
            self._kl_captured = None
            self.graph_fb = self.graph_enc = self.graph_opt = None

    def set_kl_schedule(self, fn) -> None:
        """fn(epoch) -> KL weight (hulc2_amd.kl_schedule.linear / sigmoid / constant, or any callable); begin_epoch applies it.  The rule is
        not state (as the lr schedule's function is not): a resumed run attaches the same one."""
        self._kl_schedule = fn

    def begin_epoch(self, epoch: int) -> None:
        """what the reference's on_train_epoch_start callbacks do for a Lightning loop: set the KL weight of this epoch"""
        if self._kl_schedule is not None:
            beta = self._kl_schedule(int(epoch))
            if beta is not None:                                  # (kl_schedule.constant(): the weight is never set, as in the reference)
                self.set_kl_beta(beta)

    def close(self) -> None:
        """Detach this trainer from the model (WeightKeeper.close: load hook, gradient sinks) and remove its per-parameter hooks."""
        super().close()
        for h in getattr(self, "_acc_hooks", ()):
            h.remove()
        self._acc_hooks = []
        b = getattr(self, "buckets", None)
        if b is not None:
            b.close()

    def _saw_autograd_grad(self, p) -> None:
        """post-accumulate hook: this parameter's gradient arrives through autograd's `grad +=` (not a kernel-side sink), so its arena slice must
        be zeroed before every step.  One that shows up only after the zeroing plan was made asks for a new plan — through a flag that
        optimizer_step() acts on AFTER its clean-up of this step: the backward that is running was started in overwrite mode and must be
        finished in it (clearing the plan here skipped the clean-up of planned-but-unwritten sinks for this very step)."""
        k = id(p)
        if k not in self._autograd_written:
            self._autograd_written.add(k)
            if self._zero_planned is not None and k not in self._zero_planned:
                self._replan_pending = True

    def _keep_encoder_output(self, module, inputs, output):
        self._emb = output if (self._split_active and torch.is_tensor(output) and output.requires_grad) else None

    _split_active = False

    def _forward_backward_head(self, batch, batch_idx: int, count: bool = True) -> torch.Tensor:
        """forward + backward down to the encoder output: every gradient outside the camera encoders is final afterwards"""
        shadow.bump_epoch()
        kn.advance_step_state(self.dev, True, count)
        kn.wgrad_reset(self.dev)
        self.zero_grad()
        self._split_active = True
        try:
            loss = self.model.training_step(batch, batch_idx)
        finally:
            self._split_active = False
        emb = self._emb
        if emb is None:
            raise RuntimeError("split backward: the perceptual encoder was not called exactly through its module (no output captured)")
        torch.autograd.backward(loss, grad_tensors=self._one_like(loss), inputs=[emb] + self.rest_params)
        kn.wgrad_flush(self.dev)                     # (autograd's end-of-pass callback already issued it: no-op unless the pass was cut short)
        return loss.detach()

    def _backward_encoder(self) -> None:
        emb, self._emb = self._emb, None
        g, emb.grad = emb.grad, None
        torch.autograd.backward(emb, grad_tensors=g, inputs=self.enc_params)
        kn.wgrad_flush(self.dev)

    def zero_grad(self):
        self.grads_zeroed_at = None                        # (optim.Adam.zero_grad's mark: this pass writes the arena with kernels of its own)
        self._zero_arena()
        for p, off in zip(self.params, self.offsets):      # autograd may have replaced .grad; re-point at the arena
            if p.grad is None or p.grad.data_ptr() != self.flat_g.data_ptr() + off * 4:
                p.grad = self.flat_g[off:off + p.numel()].view(p.shape)

    def optimizer_step(self):
        self._settle_sinks()
        self._optimizer_launch()

    def _optimizer_launch(self):
        """the optimizer pass over the finished gradient arena and the derived copies behind it (the settle clean-up has run)"""
        self.step_count += 1
        common = dict(grad_scale=1.0 / self.world,
                      step_state_dev=kn.step_state(self.dev),      # step count lives on the device (graph replay)
                      lo=self.flat_lo, lo_ranges=self.lo_ranges,   # (the split operands' remainders come out of the same pass)
                      lr_dev=self._lr_dev,                         # (None unless set_lr / set_lr_schedule was called)
                      **self._clip_args())                         # (gradient clipping: the norm pass runs here, in front of the step)
        if self.optimizer == "adam":
            kn.adam_step(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.flat_bf16, self.total, self.lr, self.betas[0],
                         self.betas[1], self.eps, self.wd, self.step_count, **common)
        elif self.optimizer == "adamw":
            kn.adamw_step(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.flat_bf16, self.total, self.lr, self.betas[0],
                          self.betas[1], self.eps, self.wd, self.step_count, skip_ranges=self.skip_ranges, **common)
        else:
            kn.sgd_step(self.flat_p, self.flat_g, self.exp_avg if self.exp_avg.numel() else None, self.flat_bf16, self.total, self.lr,
                        self.momentum, self.dampening, self.nesterov, self.wd, self.step_count, skip_ranges=self.skip_ranges, **common)
        self.derive_after_step()                                   # (the other derived copies: two launches behind the optimizer's)

    def _forward_backward(self, batch, batch_idx: int, count: bool = True) -> torch.Tensor:
        """count: this pass also bumps the device optimizer step count (not the later micro-batches of an accumulation window, and not the
        captured pass of one: replay() bumps the count when a window opens)"""
        shadow.bump_epoch()                    # every repack/shadow is re-made inside this step (and inside a capture)
        kn.advance_step_state(self.dev, True, count)       # fresh dropout / plan-sample stream; step count + 1 with `count`
        kn.wgrad_reset(self.dev)
        self.zero_grad()
        loss = self.model.training_step(batch, batch_idx)
        with kn.wgrad_branch_scope():          # (the recurrent weight gradients as a third branch of this graph: functional.DecoderRNNFn.backward)
            torch.autograd.backward(loss, grad_tensors=self._one_like(loss))
            kn.wgrad_flush(self.dev)
        return loss.detach()

    def _one_like(self, loss: torch.Tensor) -> torch.Tensor:
        """d loss / d loss = 1, kept per (shape, device): backward() would fill a fresh ones tensor every step"""
        one = self.__dict__.get("_one")
        if one is None or one.shape != loss.shape or one.device != loss.device or one.dtype != loss.dtype:
            one = self.__dict__["_one"] = torch.ones_like(loss)
        return one

    # Hook for processes that SHARE one GPU (tests: two gloo ranks on a one-GPU box): a context-manager factory entered around every stretch of GPU
    # work that holds no collective.  The device-wide-barrier kernels need the GPU to themselves, so such ranks take turns (a file lock that
    # synchronises the device before it is released).  Default: nothing.
    gpu_section = staticmethod(contextlib.nullcontext)
    time_comm = False              # bench.py: record an event pair around the wait for the gradient exchange (exposed communication)

    def _comm_wait_begin(self):
        if self.time_comm and self.dev.type == "cuda":
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            return ev
        return None

    def _comm_wait_end(self, ev) -> None:
        if ev is not None:
            ev[1].record()
            self._comm_events.append(ev)

    def comm_exposed_ms(self) -> float:
        """mean time per step the compute stream spent waiting for the gradient exchange since the last call (synchronises)"""
        evs, self._comm_events = self._comm_events, []
        if not evs:
            return 0.0
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in evs) / len(evs)

    def step(self, batch, batch_idx: int = 0) -> torch.Tensor:
        """zero grads -> training_step -> backward (+ overlapped all-reduce) -> fused Adam.  Returns the detached loss.
        accumulate_grad_batches > 1: one micro-batch; the exchange and the optimizer follow only the one that closes its window."""
        if self.accumulate_grad_batches > 1:
            with self.gpu_section():
                loss = self._forward_backward(batch, batch_idx, count=self.micro_batch == 0)
                self._settle_sinks()                 # its clean-up fills slices of flat_g: the accumulator reads the arena behind it
                closing = self._accumulate()
            if closing:
                self._window_tail(self._optimizer_launch)
            return loss
        with (self.gpu_section() if not (self.multi and self.buckets.overlap) else contextlib.nullcontext()):
            loss = self._forward_backward(batch, batch_idx)
        ev = self._comm_wait_begin()
        self.buckets.finish()
        self._comm_wait_end(ev)
        with self.gpu_section():
            self._apply_lr_schedule()
            self.optimizer_step()
            self._opt_steps += 1
            self._poll_faults()
        return loss

    def _window_tail(self, optimizer) -> None:
        """behind the micro-batch that closed a window (flat_g holds G): the one gradient exchange of the window, the lr write, then
        `optimizer` — the launches themselves or the captured graph's replay"""
        ev = self._comm_wait_begin()
        self.buckets.finish()
        self._comm_wait_end(ev)
        with self.gpu_section():
            self._apply_lr_schedule()
            optimizer()
            self._opt_steps += 1
            self._poll_faults()

    _since_check = 0

    def _poll_faults(self) -> None:
        """every N steps (one device sync): a barrier-kernel timeout becomes an exception; the Adam kernel has skipped the faulty steps"""
        self._since_check += 1
        if self.dev.type == "cuda" and self._since_check >= self._fault_every:
            self._since_check = 0
            try:
                kn.check_faults(self.dev)
            except Exception:
                # a timed-out chain kernel leaves its barrier counters non-zero in a workspace whose address is baked into the captured
                # graphs (or lives in their private pool): replaying them again would mis-count every barrier.  The graphs are dropped —
                # step() keeps working eagerly on fresh workspaces, replay() asks for a new capture()  
                self.graph_fb = self.graph_enc = self.graph_opt = None
                raise

    # ---- hipGraph mode: the ~900 launches of a step are captured once and replayed ----------------------
    def capture(self, batch) -> None:
        """Capture forward+backward and the optimizer as two HIP graphs over the (static, device-resident) batch.
        Between them the gradient arena is all-reduced eagerly when world > 1 (construct with overlap=False).
        Call after a few eager warm-up steps (allocator pools, lazy scratch buffers and kernels are then live).
        accumulate_grad_batches = k > 1: only at a window boundary (RuntimeError otherwise); the warm-up is two whole WINDOWS and leaves the
        trainer at a boundary.  ONE forward/backward graph serves every micro-batch — it advances the RNG word only, replay() bumps the
        step count when a window opens — and replay() launches the settle clean-up and the accumulate pass eagerly behind it (static
        pointers, no host synchronisation); the optimizer graph replays only when the window closes.  Moving through a window never drops
        or recaptures a graph; a change of k does.  Several ranks: the split replay (graph_enc) does NOT overlap the exchange with the
        encoder backward when k > 1 — on the closing micro-batch both graphs replay, the whole arena is finished, and then one exchange
        of the whole arena runs on the comm stream, as GradBuckets.finish() does it: one exchange per window instead of k."""
        assert self.dev.type == "cuda"
        k = self.accumulate_grad_batches
        if self.micro_batch != 0:
            raise RuntimeError(f"ArenaTrainer.capture: micro-batch {self.micro_batch} of {k} is open; capture at a window boundary")
        if self.multi and self.buckets.overlap:
            raise RuntimeError("graph mode needs ArenaTrainer(overlap=False): bucket hooks cannot run inside a replayed graph")
        self.comm.reserve()
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
        torch.cuda.synchronize()
        side = kn.capture_stream(self.dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                # AccumulateGrad nodes must be born on the capture stream
            for i in range(2 * k):
                self.step(batch, i)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph_fb = torch.cuda.CUDAGraph()
        # world > 1: the process group's watchdog thread may touch the runtime while this thread captures; only this thread's calls are policed
        mode = {"capture_error_mode": switches.value("CAPTURE_MODE")} if self.multi else {}
        self.graph_opt = torch.cuda.CUDAGraph()
        with kn.no_gc():                             # (no garbage collection inside a capture: see kernels.no_gc)
            if self.multi and self.enc_hi > self.enc_lo and not switches.on("NO_SPLIT_GRAPH"):
                # two graphs around the split point; replay() launches the big all-reduce between them on the comm stream
                with torch.cuda.graph(self.graph_fb, stream=side, **mode):
                    self.static_loss = self._forward_backward_head(batch, 0, count=k == 1)
                self.graph_enc = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph_enc, pool=self.graph_fb.pool(), stream=side, **mode):
                    self._backward_encoder()
            else:
                with torch.cuda.graph(self.graph_fb, stream=side, **mode):
                    self.static_loss = self._forward_backward(batch, 0, count=k == 1)
            if k > 1:
                # the settle clean-up of the captured backward, between the graphs: what it cleared, replay() clears behind every replay
                with torch.cuda.stream(side):
                    self._settle_sinks()
                self._replay_settle = tuple(self._settle_zeroed)
            with torch.cuda.graph(self.graph_opt, pool=self.graph_fb.pool(), stream=side, **mode):
                if k > 1:
                    self._optimizer_launch()
                else:
                    self.optimizer_step()
        torch.cuda.synchronize()
        # a KL weight taken by value is baked into graph_fb: replay() refuses to run it under another one
        kl = getattr(self.model, "kl_beta", None)
        self._kl_captured = None if (kl is None or getattr(self.model, "kl_beta_on_device", False)) else float(kl)
        # the regularisers (dropout probabilities of the encoders and of the decoder's RNN, l2 flags) are kernel choices and by-value arguments of graph_fb
        self._reg_captured = self._regulariser_key()

    def _regulariser_key(self):
        key = getattr(self.model, "regulariser_key", None)
        return key() if key is not None else None

    def replay(self) -> torch.Tensor:
        if self.graph_fb is None:
            raise RuntimeError("ArenaTrainer.replay: no captured graphs (never captured, or dropped after a barrier-kernel fault): call capture(batch)")
        if self._kl_captured is not None and float(self.model.kl_beta) != self._kl_captured:
            raise RuntimeError(f"ArenaTrainer.replay: the graphs were captured with kl_beta = {self._kl_captured!r} as a kernel argument and cannot "
                               f"see model.kl_beta = {float(self.model.kl_beta)!r}: set the weight through ArenaTrainer.set_kl_beta (the captured "
                               "launches then read a device scalar) and call capture() again")
        if self._regulariser_key() != self._reg_captured:
            raise RuntimeError(f"ArenaTrainer.replay: the graphs were captured with the encoder regularisers and decoder dropout "
                               f"{self._reg_captured!r} and the model now has {self._regulariser_key()!r} (dropout_vis_fc / word_dropout_p / l2 flags / "
                               "policy_rnn_dropout_p, or train / eval mode): call capture() again")
        if self.accumulate_grad_batches > 1:
            with self.gpu_section():
                if self.micro_batch == 0:            # a window opens: the optimizer step count of the pass that will close it
                    kn.step_count_advance_if(kn.step_state(self.dev))
                self.graph_fb.replay()
                if self.graph_enc is not None:
                    self.graph_enc.replay()
                for a, b in self._replay_settle:
                    self.flat_g[a:b].zero_()
                closing = self._accumulate()
            if closing:
                self._window_tail(self.graph_opt.replay)
            return self.static_loss
        with self.gpu_section():
            self.graph_fb.replay()
        if self.graph_enc is not None:
            # everything but the encoder gradients is final: reduce it on the comm stream while the conv backward graph runs
            cur, comm = torch.cuda.current_stream(), self.buckets.comm_stream
            comm.wait_stream(cur)
            with torch.cuda.stream(comm):
                for lo, hi in ((0, self.enc_lo), (self.enc_hi, self.total)):
                    self.comm.reduce(lo, hi)
            with self.gpu_section():
                self.graph_enc.replay()
            comm.wait_stream(cur)                    # the small encoder slice follows on the SAME stream: the staging buffers of the
            with torch.cuda.stream(comm):            # bf16 / direct modes are shared, two reduces must never run concurrently
                self.comm.reduce(self.enc_lo, self.enc_hi)
            ev = self._comm_wait_begin()             # (recorded behind the conv backward graph: what follows is exposed communication)
            cur.wait_stream(comm)
            self._comm_wait_end(ev)
        else:
            ev = self._comm_wait_begin()
            self.buckets.finish()
            self._comm_wait_end(ev)
        with self.gpu_section():
            self._apply_lr_schedule()                # (outside the captured region: the graph reads the device scalar)
            self.graph_opt.replay()
            self._opt_steps += 1
            self._poll_faults()
        return self.static_loss
