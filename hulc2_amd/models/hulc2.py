"""Hulc2 — the low-level policy LightningModule on MI355X kernels.

Mirrors hulc2.models.hulc2.Hulc2 (reference hulc2/models/hulc2.py:27-508) for the training path: the same 16
constructor arguments (un-instantiated configs, `_recursive_: false`), `setup_input_sizes`, `training_step`,
`lmp_train`, `compute_kl_loss`, `clip_auxiliary_loss`, `configure_optimizers`, `set_kl_beta`, the same logged
metric names and the same attribute names (hence state_dict keys); and for validation / rollout inference
(SURVEY.md §8 row f-1): `lmp_val`, `validation_step`, `reset`, `step`, `predict_with_plan`, `get_pp_plan_vision/_lang`.

Differences that do not change results:
  * the categorical plan sample can be injected through `dataset_batch["plan_idx"]` (parity tests); otherwise it
    is drawn on-device by the counter RNG (the reference uses torch.multinomial — no shared RNG stream exists).
    With the continuous distribution the injected quantity is the Gaussian noise, `dataset_batch["plan_eps"]` of shape
    (B, plan_features) (`plan_eps_pp` / `plan_eps_pr` in validation); `plan_idx` is ignored there
  * `use_for_aux_lang_loss` is applied inside the CLIP loss kernel instead of boolean-mask indexing, so the step
    has no host synchronisation (the reference's `torch.any` / dynamic shapes, hulc2.py:391-394,490-493)

The training step (`_training_step_impl`, what eager autograd, the step node and ArenaTrainer all run) is a driver over named stages:
`_step_stacked` (modalities of one shape stacked on the batch axis; `_stacked_forks` decides fan-out, branches and the stacked contrastive
head before the first launch, `_stacked_goals` / `_separate_goals` run the goal encoders) or `_step_per_modality` (everything else), each
handing a `_Part` per modality, the KL and decoder losses and `_contrastive_loss` of the parts to `_step_tail` (loss combine + logging).
"""
import contextlib
import logging
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np

import torch
import torch.nn as nn

from hulc2_amd import functional as HF
from hulc2_amd import kernels as kn
from hulc2_amd import switches
from hulc2_amd.arena import WeightKeeper
from hulc2_amd.compat import LightningModule, instantiate
from hulc2_amd.models.perceptual_encoders.concat_encoders import ConcatEncoders
from hulc2_amd.models.plan_encoders.plan_recognition_net import trunk_site
from hulc2_amd.trainer import ArenaTrainer
from hulc2_amd.utils.distributions import State

logger = logging.getLogger(__name__)


def _kernel_precision(fn):
    """Lightning (`precision: 16`, conf/trainer/play_trainer.yaml:3) calls the hooks inside `torch.autocast(fp16)`.  The kernels behind
    this module choose their own arithmetic (kernels.set_compute) and read their operands through raw pointers, so a framework op that
    autocast demoted to half would hand a kernel the wrong bytes: the hooks run with autocast off, as the reference itself does around
    `world_to_tcp_frame` (gripper_control.py:17).  A GradScaler's power-of-two loss scale passes through every backward kernel exactly."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        if torch.is_autocast_enabled():
            with torch.autocast(device_type="cuda", enabled=False):
                return fn(self, *args, **kwargs)
        return fn(self, *args, **kwargs)
    return wrapped


class _Part(NamedTuple):
    """one modality of a training step, as the contrastive loss, the scalar tail and the logging see it"""
    scope: str
    db: Dict
    goal: torch.Tensor                  # the modality's own goal rows (row0 None), or the stacked goals of all modalities
    seq_feat: torch.Tensor              # the posterior's pooled features, rows as in `goal`
    row0: Optional[int] = None          # set: `goal` / `seq_feat` are the stacked tensors and this modality's rows start here


class Hulc2(LightningModule):
    def __init__(self, perceptual_encoder, plan_proposal, plan_recognition, language_encoder, language_goal, visual_goal,
                 action_decoder, kl_beta: float, kl_balancing_mix: float, optimizer, lr_scheduler, distribution,
                 use_clip_auxiliary_loss: bool, clip_auxiliary_loss_beta: float, replan_freq: int = 30, proj_vis_lang=None):
        super().__init__()
        self.perceptual_encoder = instantiate(perceptual_encoder, device=self.device)
        self.setup_input_sizes(self.perceptual_encoder, plan_proposal, plan_recognition, visual_goal, action_decoder, distribution)
        self.dist = instantiate(distribution)
        self.plan_proposal = instantiate(plan_proposal, dist=self.dist)
        self.plan_recognition = instantiate(plan_recognition, dist=self.dist)
        self.visual_goal = instantiate(visual_goal)
        self.lang_encoder = instantiate(language_encoder) if language_encoder else None
        self.language_goal = instantiate(language_goal, lang_net=self.lang_encoder) if language_goal else None
        self.action_decoder = instantiate(action_decoder)
        self.use_clip_auxiliary_loss = use_clip_auxiliary_loss
        self.clip_auxiliary_loss_beta = clip_auxiliary_loss_beta
        if use_clip_auxiliary_loss:
            self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
            self.proj_vis_lang = instantiate(proj_vis_lang)
        self.kl_beta = kl_beta
        self.kl_balancing_mix = kl_balancing_mix
        self.modality_scope = "vis"
        self.optimizer_config = optimizer
        self.lr_scheduler = lr_scheduler
        self.save_hyperparameters()
        self.rollout_step_counter = 0
        self.replan_freq = replan_freq
        self.latent_goal = None
        self.plan = None

    @staticmethod
    def setup_input_sizes(perceptual_encoder, plan_proposal, plan_recognition, visual_goal, action_decoder, distribution):
        """hulc2.py:126-158: patch the `???` sizes of the child configs."""
        n = perceptual_encoder.latent_size
        plan_proposal.perceptual_features = n
        plan_recognition.in_features = n
        visual_goal.in_features = n
        action_decoder.perceptual_features = n
        if distribution.dist == "discrete":
            pf = distribution.class_size * distribution.category_size
        else:
            pf = distribution.plan_features
        plan_proposal.plan_features = plan_recognition.plan_features = action_decoder.plan_features = pf

    @property
    def num_training_steps(self) -> int:
        """hulc2.py:160-162: what Lightning estimates for the whole fit"""
        return int(self.trainer.estimated_stepping_batches)

    def compute_warmup(self, num_training_steps: int, num_warmup_steps) -> Tuple[int, int]:
        """hulc2.py:164-183: a negative num_training_steps is inferred from the trainer, a float num_warmup_steps is a fraction of the
        training steps; the warm-up is cut to an int."""
        from ..optim import resolve_warmup
        return resolve_warmup(num_training_steps, num_warmup_steps, lambda: self.num_training_steps)

    def configure_optimizers(self):
        """hulc2.py:185-198 (Adam lr 2e-4 + the configured lr_scheduler, stepped every optimizer step).  The native trainer
        (hulc2_amd/trainer.py) replaces this with the fused arena Adam and ArenaTrainer.set_lr_schedule; under Lightning any torch optimizer
        works (the keeper re-derives the weight copies)."""
        cfg = self.optimizer_config
        tgt = cfg.get("_target_") if hasattr(cfg, "get") else None
        drop_in = {"torch.optim.Adam": "Adam", "torch.optim.AdamW": "AdamW", "torch.optim.SGD": "SGD"}
        if tgt in drop_in and not switches.on("TORCH_ADAM"):
            # round 6: the unchanged conf/model/optimizer/adam.yaml gets the drop-in SUBCLASS (hulc2_amd/optim.py): same update rule, same
            # hyper-parameters, same state_dict layout (checkpoints interchange), isinstance(opt, torch.optim.Adam) holds; its step is one
            # launch of the arena kernel on the step node's gradient arena and takes a GradScaler's device scalars without a host
            # synchronisation; any configuration it does not cover (amsgrad, several groups, CPU, ...) runs torch.optim.Adam.step() on the
            # same state.  HULC_TORCH_ADAM=1 hands out torch's own class.  conf/model/optimizer/adamw.yaml and sgd.yaml get their drop-in
            # subclasses the same way (hulc_adamw_step / hulc_sgd_step), under the same opt-out.
            from .. import optim
            opt = getattr(optim, drop_in[tgt])(self.parameters(), **{k: v for k, v in cfg.items() if not str(k).startswith("_")})
        else:
            opt = instantiate(cfg, params=self.parameters())
        from ..optim import make_lr_scheduler
        sc = self.lr_scheduler
        if "num_warmup_steps" in sc:                        # hulc2.py:187-193: -1 training steps = the trainer's estimate, a float warm-up = a fraction
            sc["num_training_steps"], sc["num_warmup_steps"] = self.compute_warmup(sc["num_training_steps"], sc["num_warmup_steps"])
            logger.info("Inferring number of training steps, set to %d", sc["num_training_steps"])
            logger.info("Inferring number of warmup steps from ratio, set to %d", sc["num_warmup_steps"])
        sched = make_lr_scheduler(sc, opt)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": sched, "interval": "step", "frequency": 1}}

    def configure_gradient_clipping(self, optimizer, *args, gradient_clip_val=None, gradient_clip_algorithm=None, **kwargs):
        """Lightning's hook behind `trainer.gradient_clip_val` / `gradient_clip_algorithm`, called before every optimizer step.  Signatures:
        (optimizer, optimizer_idx, gradient_clip_val, gradient_clip_algorithm) in Lightning 1.x, without optimizer_idx in 2.x; the two
        values come positionally or by keyword.  A drop-in optimizer (hulc2_amd.optim.Adam / AdamW / SGD) is handed the setting
        (set_grad_clip) and clips inside its own step — one norm pass over the gradient arena and a multiplier in the step kernel, under a
        GradScaler too — so nothing is clipped here and `.grad` stays as backward left it.  Any other optimizer gets the base class's
        behaviour, self.clip_gradients(...), where the base class has it."""
        from ..optim import _ArenaStep
        rest = list(args)
        kwargs.pop("optimizer_idx", None)
        is_algo = lambda x: x is None or isinstance(x, str) or hasattr(x, "value")
        if len(rest) == 3 or (len(rest) == 2 and not is_algo(rest[1])) or (len(rest) == 1 and type(rest[0]) is int):
            rest.pop(0)                                      # Lightning 1.x: optimizer_idx (Lightning itself passes the two values by keyword)
        if rest:
            gradient_clip_val = rest.pop(0)
        if rest:
            gradient_clip_algorithm = rest.pop(0)
        algo = getattr(gradient_clip_algorithm, "value", gradient_clip_algorithm)      # (Lightning's GradClipAlgorithmType enum or a string)
        inner = getattr(optimizer, "optimizer", optimizer)   # (a LightningOptimizer wraps the torch one)
        if isinstance(inner, _ArenaStep):
            algo = "norm" if algo is None else str(algo).lower()
            if algo not in ("norm", "value"):
                raise ValueError(f"configure_gradient_clipping: gradient_clip_algorithm {algo!r} is not 'norm' or 'value'")
            val = float(gradient_clip_val) if gradient_clip_val else None
            inner.set_grad_clip(max_norm=val if algo == "norm" else None, value=val if algo == "value" else None)
            return
        base = getattr(self, "clip_gradients", None)         # (pl.LightningModule's; the stand-in module of hulc2_amd.compat has none)
        if base is not None:
            base(optimizer, gradient_clip_val=gradient_clip_val, gradient_clip_algorithm=gradient_clip_algorithm)

    # ---- hot path ----------------------------------------------------------------------------------
    @staticmethod
    def _goal_site(is_lang: bool):
        """precision scope of a goal encoder: only the LANGUAGE goal is upstream of the contrastive head — in a bf16 step the
        site "goal" makes that encoder's forward exact and leaves the visual one on its bf16 launches; 'mixed' / 'fp32' steps treat both alike"""
        if is_lang or kn.base_mode() != "bf16":
            return kn.site_scope("goal")
        return contextlib.nullcontext()

    def lmp_train(self, perceptual_emb, latent_goal, train_acts, robot_obs, plan_idx: Optional[torch.Tensor] = None,
                  plan_eps: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, State, State, torch.Tensor]:
        """hulc2.py:200-245; returns the prior/posterior *states* in place of torch.distributions objects."""
        pp_state = self.plan_proposal(perceptual_emb[:, 0], latent_goal)
        pr_state, seq_feat = self.plan_recognition(perceptual_emb, seed=trunk_site(self.modality_scope))
        site = 0xA11CE if "lang" in self.modality_scope else 0xB0B       # distinct RNG sites for the two modalities
        sampled_plan, _ = self.dist.rsample_plan(pr_state, seed=site, idx=plan_idx, eps=plan_eps)
        # (one modality's rows, restarting at 0: the decoder's RNN dropout takes the modality's own RNG site)
        action_loss = self.action_decoder.loss(sampled_plan, perceptual_emb, latent_goal, train_acts, robot_obs, modality_scope=self.modality_scope)
        kl_loss = self.compute_kl_loss(pp_state, pr_state)
        return kl_loss, action_loss, action_loss + kl_loss, pp_state, pr_state, seq_feat

    def _keep_weight_copies_fresh(self):
        """Under an EXTERNAL optimizer (Lightning + torch.optim.Adam, hulc2/training.py:79-82) nobody maintains the kernel-side copies of the
        weights (bf16 shadows, transposed tiles, packed fragments, split-operand remainders, conv repacks): shadow.weight_operand re-derives
        each of them per parameter and layout with torch ops when the parameter's version has changed — ~200 small launches per step.  The
        first training-mode step on a GPU without an ArenaTrainer therefore installs a WeightKeeper (hulc2_amd/arena.py): the parameters move into
        one arena (same Parameter objects, same values: optimizers, DDP and checkpoints are unaffected) and all copies are re-made by five
        launches whenever the optimizer has stepped.  bf16 arithmetic modes only; HULC_NO_AUTO_SHADOWS=1 keeps the lazy per-parameter path.
        Round 5: the keeper also owns the gradient arena of the step node (hulc2_amd/stepnode.py; HULC_NO_STEP_NODE=1: weight copies only).
        Returns the keeper when it is this model's (else None: a full ArenaTrainer drives the step, or the lazy path is selected)."""
        if kn.base_mode() == "fp32" or switches.on("NO_AUTO_SHADOWS"):
            return None
        ref = self.__dict__.get("_hulc_arena_trainer")
        tr = ref() if ref is not None else None
        if tr is not None and tr.model is not self:               # (a deep copy of a model carries the original's weak reference along)
            tr = None
        if tr is None:
            # the model owns its keeper (a deepcopy of the model gets None here and builds its own)
            tr = self.__dict__["_hulc_shadow_keeper"] = WeightKeeper(self, step_node=not switches.on("NO_STEP_NODE"))
        if not isinstance(tr, ArenaTrainer):
            tr.refresh_if_stale()
            return tr
        return None

    def _fresh_weight_copies(self) -> None:
        """every forward entry point that is NOT a training step (validation, rollout): under an external optimizer the keeper's copies are
        re-derived when a parameter has been written since (optimizer.step(), an EMA swap, weight surgery) — the arena views the kernels
        read carry no version of their own"""
        tr = self.__dict__.get("_hulc_shadow_keeper")
        if tr is not None:                                        # (only ever a WeightKeeper: _keep_weight_copies_fresh put it there)
            ref = self.__dict__.get("_hulc_arena_trainer")
            if ref is not None and ref() is tr:
                tr.refresh_if_stale()

    def _step_node(self, keeper):
        """the whole training step as one autograd node (hulc2_amd/stepnode.py) when this model's keeper owns a gradient arena and the call can
        take it: gradients enabled, the keeper's parameter set still the trainable one.  Gradients still attached from earlier calls (accumulation,
        `zero_grad(set_to_none=False)`) do not keep a call off the node: it adds them back, the capturing call included (stepnode._capture)"""
        if keeper is None or not getattr(keeper, "step_node", False) or not torch.is_grad_enabled():
            return None
        node = self.__dict__.get("_hulc_step_node")
        if node is None or node.keeper is not keeper:
            from ..stepnode import StepNode
            node = self.__dict__["_hulc_step_node"] = StepNode(self, keeper)
        return node if node.usable() else None

    @_kernel_precision
    def training_step(self, batch: Dict[str, Dict], batch_idx: int) -> torch.Tensor:
        """hulc2.py:336-442."""
        node = None
        if self.training:
            # every training-mode call draws fresh dropout masks and a fresh latent-plan sample (the device RNG word, kernels.step_state),
            # under any trainer: Lightning + a torch optimizer never touches that word, ArenaTrainer marks it fresh for this step itself
            p0 = next(self.parameters())
            if p0.is_cuda:
                node = self._step_node(self._keep_weight_copies_fresh())
                if node is None:                               # (the step node walks the word itself: inside its captured forward graph)
                    kn.ensure_fresh_rng(p0.device)
        else:
            self._fresh_weight_copies()
        # under an external optimizer (Lightning's loop, hulc2/training.py:79-82) the step is ONE autograd node — eager at first, two replayed
        # hipGraphs from the third step of a configuration on (hulc2_amd/stepnode.py); otherwise the Functions of functional.py hang on the loss
        total_loss, logs = node(batch, batch_idx) if node is not None else self._training_step_impl(batch, batch_idx)
        for name, value, kw in logs:
            self.log(name, value, **kw)
        return total_loss

    def _training_step_impl(self, batch: Dict[str, Dict], batch_idx: int):
        """the arithmetic of training_step: -> (total loss, [(logged name, value, self.log keyword arguments)]).  Encoders, goal, prior /
        posterior, latent plan sample, KL, decoder (hulc2.py:380-386,228-242): modalities of identical shape are stacked on the batch axis
        through every shared network (same per-row arithmetic, half the launches; only the goal encoders differ per modality, and every
        loss is still the mean over its own modality's rows), any other batch runs one modality after the other."""
        mods = list(batch.items())
        parts, kl_vec, act_losses, clip = self._step_stacked(mods) if self._batchable(mods) else self._step_per_modality(mods)
        return self._step_tail(parts, kl_vec, act_losses, clip)

    def _stacked_forks(self, mods, B: int):
        """How the stacked step is arranged, decided before its first launch: -> (fan, fork, fork_post, stacked_head, fork_clip)
          fan           the embedding's four consumers get their views from one fan-out node (one gather launch forward, ONE merge launch
                        backward instead of autograd's select / slice backward fills and three accumulate adds): emb[:, 0] -> prior,
                        emb[:B, -1] of the leading vision modality -> visual goal encoder, emb -> posterior, emb[..., lo:hi] time-major ->
                        action decoder.  Needs a GPU model and the vision modality in front of the language ones.
          fork          the step's independent branches run on a side stream eagerly and as branches of the captured graph in replay; autograd
                        runs each branch's backward on the stream of its forward, so the backward forks the same way.  HULC_FORK=0: one
                        after the other.
          fork_post     round 6: the posterior (transformer trunk + its head) does not depend on the goal encoders and the prior
                        (hulc2.py:228-233): it is the first branch.  Both sides are cooperative launches that own a CU per workgroup: each
                        keeps to half of the device (kernels.coop_share_scope -> coop_share of the launches' descriptors,
                        include/hulc2_amd.h).  A RECURRENT posterior (plan_recognition=birnn) is no branch: its persistent sweeps own every
                        CU behind a device-wide barrier, and spinning beside the prior's cooperative chain on a side stream they would time
                        out.  It runs on the main stream, after the prior, outside coop_share_scope(2).
          stacked_head  the contrastive head sees the stacked rows when the language modality is the last segment: rows below row0 are masked
                        out inside the loss kernel (their gradient is exactly zero) — no slice of the pooled features / goals, no gradient
                        scatter on the way back
          fork_clip     round 6: the contrastive head (two projections + the loss, forward and backward ~0.15 ms of small launches) needs
                        the pooled posterior features and the goals only — it is the second branch, beside sample / KL / the decoder's input
                        projections, and its backward beside the start of the decoder's.  The recurrent sweeps take every CU while they run,
                        so nothing in this branch may be a cooperative launch (coop_share_scope(0): the projections' chains fall back to
                        GEMMs — a chain spinning on some CUs while the sweep waits for all of them would never finish)."""
        lang_ix = [i for i, (sc, _) in enumerate(mods) if "lang" in sc]
        vis_first = "lang" not in mods[0][0] and all("lang" in sc for sc, _ in mods[1:])
        fan = vis_first and next(self.parameters()).is_cuda
        fork = fan and kn.fork_branches()
        fork_post = fork and not getattr(self.plan_recognition, "recurrent", False)
        stacked_head = fan and lang_ix == [len(mods) - 1] and self.use_clip_auxiliary_loss and len(mods) * B <= 128
        fork_clip = fork and self.use_clip_auxiliary_loss and bool(lang_ix)
        return fan, fork, fork_post, stacked_head, fork_clip

    def _step_stacked(self, mods):
        """all modalities stacked on the batch axis: -> (parts, kl (n,), action losses (n,), contrastive loss or None)"""
        n, B = len(mods), mods[0][1]["actions"].shape[0]
        fan, fork, fork_post, stacked_head, fork_clip = self._stacked_forks(mods, B)
        with kn.site_scope("enc"):
            emb_all = self.perceptual_encoder([db["rgb_obs"] for _, db in mods], None, None)
        # (vis_in, what the visual goal encoder reads: the leading modality's last frame from the fan-out, else every modality's own rows)
        if fan:
            emb0, vis_in, emb_rec, emb_dec = HF.EmbFanoutFn.apply(emb_all, B, *self.action_decoder.perceptual_emb_slice)
        else:
            vis_in = [emb_all[i * B:(i + 1) * B] for i in range(n)]
            emb0, emb_rec, emb_dec = emb_all[:, 0], emb_all, emb_all
        cur, side = (torch.cuda.current_stream(emb_all.device), kn.branch_stream(emb_all.device)) if fork else (None, None)
        if fork_post:
            with kn.fork(cur, side, share=2):
                pr_all, seq_all = self.plan_recognition(emb_rec)
        with kn.coop_share_scope(2 if fork_post else 1):      # (the prior branch's chain launches: half of the device next to the posterior's)
            if fan:
                goal_all, goals = self._stacked_goals(mods, vis_in), None
            else:
                goals = self._separate_goals(mods, vis_in)
                goal_all = torch.cat(goals, dim=0)
            with kn.site_scope("prior"):
                pp_all = self.plan_proposal(emb0, goal_all)
        if fork_post:
            kn.join(cur, side, self.dist.state_tensor(pr_all), seq_all)       # sample + KL consume both branches
        else:
            pr_all, seq_all = self.plan_recognition(emb_rec)
        parts = []
        for i, (self.modality_scope, db) in enumerate(mods):
            if stacked_head and "lang" in self.modality_scope:
                parts.append(_Part(self.modality_scope, db, goal_all, seq_all, row0=i * B))
            else:
                parts.append(_Part(self.modality_scope, db, goals[i] if goals is not None else goal_all[i * B:(i + 1) * B],
                                   seq_all[i * B:(i + 1) * B]))
        if fork_clip:
            with kn.fork(cur, side, share=0):
                clip = self._contrastive_loss(parts)
        # sample, KL and decoder once over the stacked rows; the KL / decoder kernels return one mean per modality.  Sample + KL are ONE
        # autograd node (both consume the posterior's logits: their gradients meet inside the kernels, not in a fan-in add)
        # (injected sample, parity tests: class indices for the categorical plan, Gaussian noise for the continuous one)
        cont = self.dist.dist == "continuous"
        inj = [db.get("plan_eps" if cont else "plan_idx") for _, db in mods]
        inj_all = torch.cat(inj, dim=0) if all(i is not None for i in inj) else None
        plan_all, _, kls = self.dist.rsample_plan_and_kl(pp_all, pr_all, 0xA11CE, None if cont else inj_all, self._kl_beta_arg(),
                                                         self.kl_balancing_mix, n, eps=inj_all if cont else None)
        act_losses = self.action_decoder.loss_stacked(plan_all, emb_dec, goal_all, [db["actions"] for _, db in mods],
                                                      [db["state_info"]["robot_obs"] for _, db in mods], n, emb_tm=fan)
        if fork_clip:
            kn.join(cur, side, clip)
        else:
            clip = self._contrastive_loss(parts)
        return parts, kls, act_losses, clip

    def _stacked_goals(self, mods, emb_last):
        """The goal encoders of the stacked step behind the fan-out -> the stacked goal tensor (n * B, latent_goal_features).  The encoders stop in
        front of their LayerNorms, which then write the rows of the stacked tensor directly (one layer_norm_cat launch: no concatenation, no
        strided gradient slices on the way back).  What runs in front of it:
          * a bf16 step with site "goal" and two modalities (selective precision, DESIGN §5: of the goal encoders only the LANGUAGE one is
            upstream of the contrastive head): both encoders in ONE dual_mlp launch, the language one from split operands (three MFMAs per
            product: fp32-class values) while the visual one stays on bf16 operands ...
          * ... or, where the pair does not fit that launch: the visual encoder's own bf16 chain launch and the language encoder on the
            exact-fp32 GEMMs
          * any other step with two modalities: the two MLPs (same hidden widths, their own weights) as one plain dual_mlp launch each way
          * more than two modalities: every encoder's own launches"""
        vis, lang = self.visual_goal, self.language_goal
        if kn.base_mode() == "bf16" and kn.get_compute() == "bf16" and "goal" in kn.fp32_sites() and len(mods) == 2:
            pre = HF.dual_mlp(emb_last, vis.mlp_layers(), lang.embed(mods[1][1]["lang"]), lang.mlp_layers(), exact_b=True)
            if pre is None:
                pre_v = vis(emb_last, pre_ln=True)
                with kn.site_scope("goal"):
                    pre = (pre_v, lang(mods[1][1]["lang"], pre_ln=True))
        elif len(mods) == 2:
            with kn.site_scope("goal"):
                pre = HF.dual_mlp(emb_last, vis.mlp_layers(), lang.embed(mods[1][1]["lang"]), lang.mlp_layers())
        else:
            with kn.site_scope("goal"):
                pre = [lang(db["lang"], pre_ln=True) if "lang" in scope else vis(emb_last, pre_ln=True) for scope, db in mods]
        encs = [lang if "lang" in scope else vis for scope, _ in mods]
        with kn.site_scope("goal"):
            return HF.layer_norm_cat(list(pre), [g.ln for g in encs], dim=0, l2=[g.l2_normalize_output for g in encs])

    def _separate_goals(self, mods, embs):
        """the goal encoders of the stacked step without the fan-out: each whole, on its own modality's rows -> one goal tensor per modality"""
        goals = []
        for (scope, db), emb in zip(mods, embs):
            with self._goal_site("lang" in scope):
                goals.append(self.language_goal(db["lang"]) if "lang" in scope else self.visual_goal(emb[:, -1]))
        return goals

    def _step_per_modality(self, mods):
        """one modality after the other through the encoders, the prior and the posterior (a single modality, shapes that differ,
        HULC_NO_MODALITY_BATCHING=1): -> (parts, kl (n,), action losses (n,), contrastive loss or None)"""
        parts, embs, plans, kls = [], [], [], []
        for self.modality_scope, db in mods:
            is_lang = "lang" in self.modality_scope
            with kn.site_scope("enc"):
                emb = self._encode_modality(db)
            with self._goal_site(is_lang):
                latent_goal = self.language_goal(db["lang"]) if is_lang else self.visual_goal(emb[:, -1])
            with kn.site_scope("prior"):
                pp_state = self.plan_proposal(emb[:, 0], latent_goal)
            pr_state, seq_feat = self.plan_recognition(emb, seed=trunk_site(self.modality_scope))
            plan, _ = self.dist.rsample_plan(pr_state, seed=0xA11CE if is_lang else 0xB0B, idx=db.get("plan_idx"), eps=db.get("plan_eps"))
            kls.append(self.compute_kl_loss(pp_state, pr_state))
            parts.append(_Part(self.modality_scope, db, latent_goal, seq_feat))
            embs.append(emb)
            plans.append(plan)
        # the action decoder sees all modalities at once (shared weights, independent sequences); it returns one loss per
        # modality, each the mean over that modality's own tokens as in the reference (hulc2.py:239-241)
        act_losses = self.action_decoder.loss_segments(plans, embs, [p.goal for p in parts], [p.db["actions"] for p in parts],
                                                       [p.db["state_info"]["robot_obs"] for p in parts], scopes=[p.scope for p in parts])
        clip = self._contrastive_loss(parts)
        return parts, torch.stack([kl.reshape(()) for kl in kls]), act_losses, clip

    def _contrastive_loss(self, parts):
        """clip_auxiliary_loss summed over the language modalities; None when the loss is off or the batch has no language modality"""
        loss = None
        if self.use_clip_auxiliary_loss:
            for p in parts:
                if "lang" in p.scope:
                    term = self.clip_auxiliary_loss(p.seq_feat, p.goal, p.db["use_for_aux_lang_loss"], row0=p.row0 or 0)
                    loss = term if loss is None else loss + term
        return loss

    def _step_tail(self, parts, kl_vec, act_losses, clip):
        """the scalar tail (hulc2.py:400-430), one launch per direction: total = (sum act + sum kl) / n + beta * clip; and what the step logs"""
        act_vec = act_losses if act_losses.dim() == 1 else act_losses.reshape(-1)
        total_loss, logs = HF.LossCombineFn.apply(kl_vec, act_vec, clip, float(self.clip_auxiliary_loss_beta))
        kl_d, act_d = kl_vec.detach(), act_vec.detach()
        logged = []
        total_bs = 0
        for i, p in enumerate(parts):
            bs = p.db["actions"].shape[0]
            total_bs += bs
            logged.append((f"train/kl_loss_scaled_{p.scope}", kl_d[i], dict(on_step=False, on_epoch=True, batch_size=bs)))
            logged.append((f"train/action_loss_{p.scope}", act_d[i], dict(on_step=False, on_epoch=True, batch_size=bs)))
            logged.append((f"train/total_loss_{p.scope}", logs[3 + i], dict(on_step=False, on_epoch=True, batch_size=bs)))
        if clip is not None:
            # hulc2.py:391-394: the epoch mean of train/lang_clip_loss is weighted by the number of masked-in rows (1 when there are none) —
            # counted by the loss kernel, a device value (no torch.any / torch.sum host round trip)
            logged.append(("train/lang_clip_loss", logs[2], dict(on_step=False, on_epoch=True, batch_size=self._aux_lang_rows, sync_dist=True)))
        logged.append(("train/kl_loss", logs[0], dict(on_step=False, on_epoch=True, batch_size=total_bs)))
        logged.append(("train/action_loss", logs[1], dict(on_step=False, on_epoch=True, batch_size=total_bs)))
        logged.append(("train/total_loss", total_loss, dict(on_step=False, on_epoch=True, batch_size=total_bs)))
        return total_loss, logged

    def _encode_modality(self, db):
        """the perceptual encoder on ONE modality's frames (rows restart at 0 per call): ConcatEncoders hands the camera heads' fc dropout
        the modality's own RNG site, so vis and lang draw different masks; other encoder classes take the reference's three arguments"""
        if isinstance(self.perceptual_encoder, ConcatEncoders):
            return self.perceptual_encoder(db["rgb_obs"], db["depth_obs"], db["robot_obs"], modality_scope=self.modality_scope)
        return self.perceptual_encoder(db["rgb_obs"], db["depth_obs"], db["robot_obs"])

    def regulariser_key(self) -> tuple:
        """the regularisers a captured step has baked in as kernel choices and arguments (dropout_vis_fc of both cameras, word_dropout_p, the
        four l2 flags and, as the last element, the decoder's effective policy_rnn_dropout_p: 0.0 in eval mode): part of what keys a captured
        graph (StepNode._signature, ArenaTrainer.capture / replay)"""
        key = []
        enc = self.perceptual_encoder
        for name in ("rgb_static_encoder", "rgb_gripper_encoder"):
            e = getattr(enc, name, None)
            key.append((float(getattr(e, "drop_p", 0.0)), bool(getattr(e, "l2_normalize_output", False))) if e is not None else None)
        key.append(bool(getattr(self.visual_goal, "l2_normalize_output", False)))
        lg = self.language_goal
        if lg is not None:
            m0 = lg.mlp[0] if hasattr(lg, "mlp") else None
            key.append((float(m0.p) if (isinstance(m0, nn.Dropout) and lg.training) else 0.0, bool(getattr(lg, "l2_normalize_output", False))))
        dec = self.action_decoder
        key.append(float(getattr(dec, "policy_rnn_dropout_p", 0.0)) if dec.training else 0.0)
        return tuple(key)

    @staticmethod
    def _batchable(mods) -> bool:
        """all modalities carry the same cameras and tensor shapes (the CALVIN vis/lang batches do)"""
        if len(mods) < 2 or switches.on("NO_MODALITY_BATCHING"):
            return False
        ref = mods[0][1]
        for _, db in mods[1:]:
            if db["actions"].shape != ref["actions"].shape or set(db["rgb_obs"]) != set(ref["rgb_obs"]):
                return False
            if any(db["rgb_obs"][k].shape != ref["rgb_obs"][k].shape for k in ref["rgb_obs"]):
                return False
        return True

    def compute_kl_loss(self, pp_state: State, pr_state: State) -> torch.Tensor:
        """hulc2.py:444-466."""
        return self.dist.kl_balanced(pp_state, pr_state, self._kl_beta_arg(), self.kl_balancing_mix)

    _kl_beta_dev = None            # one fp32 element on the parameters' device once set_kl_beta() was called on a GPU model (device-beta mode)

    def set_kl_beta(self, kl_beta):
        """hulc2.py `set_kl_beta` (driven every epoch by hulc2/utils/kl_callbacks.py).  `self.kl_beta` stays the Python float.  On a GPU model
        the value (rounded to fp32 as the kernel argument would be) is also written into a one-element device tensor with one stream-ordered
        fill on the current stream — no host synchronisation — and from the first call on the KL kernels read THAT word instead of taking beta
        by value: a captured step follows the annealing without a recapture.  The tensor is a plain attribute (no buffer, no parameter: the
        checkpoint keys are unchanged).  Call it between steps: a value written between a forward and its backward is undefined."""
        dev = self._param_device()
        if dev is not None and dev.type == "cuda":
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("Hulc2.set_kl_beta was called while a stream capture is in progress: the fill would become a node of the "
                                   "graph and every replay would write this value back — set the KL weight between captures / replays")
            self._kl_beta_fill(dev, kl_beta)
        self.kl_beta = kl_beta

    def _param_device(self):
        p = next(self.parameters(), None)
        return p.device if p is not None else None

    _kl_beta_word = None           # the fp32 value last written into _kl_beta_dev (host copy: comparing costs no synchronisation)

    def _kl_beta_fill(self, dev, kl_beta):
        import ctypes
        if self._kl_beta_dev is None or self._kl_beta_dev.device != dev:
            self._kl_beta_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self._kl_beta_word = ctypes.c_float(float(kl_beta)).value
        self._kl_beta_dev.fill_(self._kl_beta_word)

    def _kl_beta_arg(self):
        """what the distribution's KL entry points get: the float (by value, as before any set_kl_beta call and on a CPU model) or, in
        device-beta mode, the device word.  The word is written again here when it no longer holds fp32(self.kl_beta) — set_kl_beta ran while
        the model was on the CPU and the model came back — and made anew when the model has moved to another device."""
        if self._kl_beta_dev is None:
            return self.kl_beta
        dev = self._param_device()
        if dev is None or dev.type != "cuda":
            return self.kl_beta
        import ctypes
        if self._kl_beta_dev.device != dev or self._kl_beta_word != ctypes.c_float(float(self.kl_beta)).value:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("Hulc2: the device word of kl_beta is out of date inside a stream capture; call set_kl_beta on the GPU model "
                                   "before capturing")
            self._kl_beta_fill(dev, self.kl_beta)
        return self._kl_beta_dev

    @property
    def kl_beta_on_device(self) -> bool:
        """device-beta mode: set_kl_beta() has been called on a GPU model and the model is on a GPU now — the KL kernels read the device word"""
        if self._kl_beta_dev is None:
            return False
        dev = self._param_device()
        return dev is not None and dev.type == "cuda"

    def clip_auxiliary_loss(self, seq_vis_feat, encoded_lang, use_for_aux_loss, row0: int = 0):
        """hulc2.py:472-508; rows with use_for_aux_loss == False are excluded inside the kernel.  row0 > 0: the features are the stacked rows of
        several modalities, the flags describe rows row0 .. and the rows below never take part."""
        if use_for_aux_loss is None:
            use_for_aux_loss = torch.ones(seq_vis_feat.shape[0] - row0, dtype=torch.bool, device=seq_vis_feat.device)
        with kn.site_scope("head"):              # exact-fp32 projections inside a bf16 step (selective precision)
            im, tx = self.proj_vis_lang(seq_vis_feat, encoded_lang)
            loss, self._aux_lang_rows = HF.ClipLossFn.apply(im, tx, use_for_aux_loss, self.logit_scale, int(row0))
            return loss

    # ---- validation and rollout inference on the same kernels ------------------------
    _plan_calls = 0

    def _sample_plan(self, state: State, idx: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dist.sample_latent_plan(dist.get_dist(state)) (distributions.py:23-35, hulc2.py:287,302): a one-hot draw per category (a Gaussian
        draw for the continuous plan), no gradient.  A fresh counter-RNG stream per call; `idx` injects the class indices, `eps` the
        Gaussian noise (parity tests)."""
        Hulc2._plan_calls += 1
        with torch.no_grad():
            plan, _ = self.dist.rsample_plan(state, seed=0xC0FFEE00 + Hulc2._plan_calls, idx=idx, eps=eps)
        return plan

    @torch.no_grad()
    def lmp_val(self, perceptual_emb, latent_goal, actions, robot_obs, plan_idx_pp=None, plan_idx_pr=None, plan_eps_pp=None, plan_eps_pr=None):
        """hulc2.py:247-334: plans sampled from the prior and the posterior, decoder loss + one sampled action sequence for each,
        KL, per-dimension mean absolute errors and gripper success rates."""
        def metrics(sample_act):
            mae = torch.mean(torch.abs(sample_act[..., :-1] - actions[..., :-1]), 1)             # (batch, 6)
            grip = torch.where(sample_act[..., -1] > 0, 1.0, -1.0)
            return mae, torch.mean((actions[..., -1] == grip).float())

        pp_state = self.plan_proposal(perceptual_emb[:, 0], latent_goal)
        sampled_plan_pp = self._sample_plan(pp_state, plan_idx_pp, plan_eps_pp)
        action_loss_pp, sample_act_pp = self.action_decoder.loss_and_act(sampled_plan_pp, perceptual_emb, latent_goal, actions, robot_obs)
        mae_pp, gripper_sr_pp = metrics(sample_act_pp)
        pr_state, seq_feat = self.plan_recognition(perceptual_emb)
        sampled_plan_pr = self._sample_plan(pr_state, plan_idx_pr, plan_eps_pr)
        action_loss_pr, sample_act_pr = self.action_decoder.loss_and_act(sampled_plan_pr, perceptual_emb, latent_goal, actions, robot_obs)
        mae_pr, gripper_sr_pr = metrics(sample_act_pr)
        kl_loss = self.compute_kl_loss(pp_state, pr_state)
        return (sampled_plan_pp, action_loss_pp, sampled_plan_pr, action_loss_pr, kl_loss, mae_pp, mae_pr, gripper_sr_pp, gripper_sr_pr,
                seq_feat)

    @_kernel_precision
    @torch.no_grad()
    def validation_step(self, batch: Dict[str, Dict], batch_idx: int) -> Dict[str, torch.Tensor]:
        """hulc2.py:510-598: same logged names, returns the sampled plans and episode indices per modality."""
        self._fresh_weight_copies()
        output = {}
        val_total_act_loss_pp = None
        for self.modality_scope, db in batch.items():
            emb = self.perceptual_encoder(db["rgb_obs"], db["depth_obs"], db["robot_obs"])
            latent_goal = self.language_goal(db["lang"]) if "lang" in self.modality_scope else self.visual_goal(emb[:, -1])
            (plan_pp, act_loss_pp, plan_pr, act_loss_pr, kl_loss, mae_pp, mae_pr, grip_pp, grip_pr, seq_feat) = self.lmp_val(
                emb, latent_goal, db["actions"], db["state_info"]["robot_obs"], db.get("plan_idx_pp"), db.get("plan_idx_pr"),
                db.get("plan_eps_pp"), db.get("plan_eps_pr"))
            if "lang" in self.modality_scope and self.use_clip_auxiliary_loss:
                self.log("val/val_pred_clip_loss", self.clip_auxiliary_loss(seq_feat, latent_goal, db["use_for_aux_lang_loss"]), sync_dist=True)
            val_total_act_loss_pp = act_loss_pp if val_total_act_loss_pp is None else val_total_act_loss_pp + act_loss_pp
            m = self.modality_scope
            self.log(f"val_total_mae/{m}_total_mae_pr", mae_pr.mean(), sync_dist=True)
            self.log(f"val_total_mae/{m}_total_mae_pp", mae_pp.mean(), sync_dist=True)
            self.log(f"val_pos_mae/{m}_pos_mae_pr", mae_pr[..., :3].mean(), sync_dist=True)
            self.log(f"val_pos_mae/{m}_pos_mae_pp", mae_pp[..., :3].mean(), sync_dist=True)
            self.log(f"val_orn_mae/{m}_orn_mae_pr", mae_pr[..., 3:6].mean(), sync_dist=True)
            self.log(f"val_orn_mae/{m}_orn_mae_pp", mae_pp[..., 3:6].mean(), sync_dist=True)
            self.log(f"val_kl/{m}_kl_loss", kl_loss, sync_dist=True)
            self.log(f"val_act/{m}_act_loss_pp", act_loss_pp, sync_dist=True)
            self.log(f"val_act/{m}_act_loss_pr", act_loss_pr, sync_dist=True)
            self.log(f"val_grip/{m}_grip_sr_pr", grip_pr, sync_dist=True)
            self.log(f"val_grip/{m}_grip_sr_pp", grip_pp, sync_dist=True)
            n_mod = len(getattr(getattr(getattr(self, "trainer", None), "datamodule", None), "modalities", None) or batch)
            self.log("val_act/action_loss_pp", val_total_act_loss_pp / n_mod, sync_dist=True)
            output[f"sampled_plan_pp_{m}"] = plan_pp
            output[f"sampled_plan_pr_{m}"] = plan_pr
            output[f"idx_{m}"] = db["idx"]
        return output

    def reset(self):
        """hulc2.py:600-606: call at the beginning of a rollout."""
        self.plan = None
        self.latent_goal = None
        self.rollout_step_counter = 0

    @_kernel_precision
    def step(self, obs, goal):
        """hulc2.py:608-628: one control step; a new plan is sampled from the prior every `replan_freq` steps."""
        if self.rollout_step_counter % self.replan_freq == 0:
            if "lang" in goal:
                self.plan, self.latent_goal = self.get_pp_plan_lang(obs, goal)
            else:
                self.plan, self.latent_goal = self.get_pp_plan_vision(obs, goal)
        action = self.predict_with_plan(obs, self.latent_goal, self.plan)
        self.rollout_step_counter += 1
        return action

    @torch.no_grad()
    def predict_with_plan(self, obs, latent_goal, sampled_plan):
        """hulc2.py:630-652."""
        self._fresh_weight_copies()
        emb = self.perceptual_encoder(obs["rgb_obs"], obs["depth_obs"], obs["robot_obs"])
        return self.action_decoder.act(sampled_plan, emb, latent_goal, obs["robot_obs_raw"])

    @torch.no_grad()
    def get_pp_plan_vision(self, obs: dict, goal: dict):
        """hulc2.py:654-683: current and goal frames as a 2-step sequence through the encoders, plan from the prior."""
        assert len(obs["rgb_obs"]) == len(goal["rgb_obs"])
        self._fresh_weight_copies()
        imgs = {k: torch.cat([v, goal["rgb_obs"][k]], dim=1) for k, v in obs["rgb_obs"].items()}     # (1, 2, C, H, W)
        state = torch.cat([obs["robot_obs"], goal["robot_obs"]], dim=1) if "robot_obs" in obs and "robot_obs" in goal else None
        emb = self.perceptual_encoder(imgs, {}, state)
        latent_goal = self.visual_goal(emb[:, -1])
        sampled_plan = self._sample_plan(self.plan_proposal(emb[:, 0], latent_goal))
        self.action_decoder.clear_hidden_state()
        return sampled_plan, latent_goal

    @torch.no_grad()
    def get_pp_plan_lang(self, obs: dict, goal: dict):
        """hulc2.py:685-707."""
        self._fresh_weight_copies()
        emb = self.perceptual_encoder(obs["rgb_obs"], obs["depth_obs"], obs["robot_obs"])
        latent_goal = self.language_goal(goal["lang"])
        sampled_plan = self._sample_plan(self.plan_proposal(emb[:, 0], latent_goal))
        self.action_decoder.clear_hidden_state()
        return sampled_plan, latent_goal

    def on_train_epoch_start(self) -> None:
        logger.info("Start training epoch %s", getattr(self, "current_epoch", "?"))

    def on_train_epoch_end(self, unused=None) -> None:
        logger.info("Finished training epoch %s", getattr(self, "current_epoch", "?"))

    def on_validation_epoch_end(self) -> None:
        logger.info("Finished validation epoch %s", getattr(self, "current_epoch", "?"))
