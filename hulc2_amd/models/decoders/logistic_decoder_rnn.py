"""Action decoder: 2-layer ReLU RNN + discretised logistic mixture / gripper heads.

Mirrors hulc2.models.decoders.logistic_decoder_rnn.LogisticDecoderRNN (reference logistic_decoder_rnn.py:27-284):
same 19 constructor kwargs, same parameter/buffer names (rnn.*, mean_fc, log_scale_fc, prob_fc, gripper_fc,
one_hot_embedding_eye, ones, gripper_bounds, action_{max,min}_bound).  nn.RNN is only the parameter container.
Training path (`loss`) = DecoderRNNFn -> one fused head GEMM (182 outputs, padded to 184) -> MixLossFn.
"""
from typing import List, Optional, Tuple, Union

import torch
import torch.nn as nn

from hulc2_amd import functional as HF
from hulc2_amd import gradsink
from hulc2_amd.models.decoders.action_decoder import ActionDecoder
from hulc2_amd.models.perceptual_encoders.vision_network import check_dropout_p, fc_site

# Dropout sites of policy_rnn_dropout_p, after vision_network's pattern: functional.DECODER_RNN_SITE (0x5EED7001) for the stacked call, the
# modality's own where a modality runs a call of its own (Hulc2.lmp_train; Hulc2._step_per_modality with unequal batches: the separate passes of
# loss_segments), whose rows restart at 0.
DECODER_RNN_MODALITY_SITES = {"vis": 0x5EED7101, "lang": 0x5EED7201}


class LogisticDecoderRNN(ActionDecoder):
    def __init__(self, perceptual_features: int, latent_goal_features: int, plan_features: int, n_mixtures: int, hidden_size: int,
                 out_features: int, log_scale_min: float, act_max_bound: Union[List[float], tuple], act_min_bound: Union[List[float], tuple],
                 dataset_dir: str, load_action_bounds: bool, num_classes: int, gripper_alpha: float, perceptual_emb_slice: tuple,
                 policy_rnn_dropout_p: float, num_layers: int, rnn_model: str, gripper_control: bool, discrete_gripper: bool):
        super().__init__()
        if rnn_model != "rnn_decoder" or num_layers != 2 or not discrete_gripper:
            raise NotImplementedError("configured path: 2-layer ReLU rnn_decoder, discrete gripper "
                                      "(conf/model/action_decoder/logistic_decoder_rnn_calvin.yaml)")
        policy_rnn_dropout_p = check_dropout_p(policy_rnn_dropout_p, "policy_rnn_dropout_p")
        self.policy_rnn_dropout_p = policy_rnn_dropout_p      # nn.RNN(dropout=p): layer 1 reads a dropped h0_t while the module trains
        if load_action_bounds:
            raise NotImplementedError("load_action_bounds reads dataset statistics (file IO outside the hot path); "
                                      "pass the bounds in the config")
        self.n_dist = n_mixtures
        self.gripper_control, self.discrete_gripper = gripper_control, discrete_gripper
        self.log_scale_min, self.num_classes, self.plan_features = log_scale_min, num_classes, plan_features
        self.perceptual_emb_slice = tuple(int(v) for v in perceptual_emb_slice)
        in_features = (self.perceptual_emb_slice[1] - self.perceptual_emb_slice[0]) + latent_goal_features + plan_features
        self.out_features = out_features - 1
        self.gripper_alpha = gripper_alpha
        self.rnn = nn.RNN(input_size=in_features, hidden_size=hidden_size, num_layers=num_layers, nonlinearity="relu",
                          bidirectional=False, batch_first=True, dropout=policy_rnn_dropout_p)
        self.mean_fc = nn.Linear(hidden_size, self.out_features * self.n_dist)
        self.log_scale_fc = nn.Linear(hidden_size, self.out_features * self.n_dist)
        self.prob_fc = nn.Linear(hidden_size, self.out_features * self.n_dist)
        self.register_buffer("one_hot_embedding_eye", torch.eye(self.n_dist))
        self.register_buffer("ones", torch.ones(1, 1, self.n_dist))
        amax, amin = list(act_max_bound), list(act_min_bound)
        self.register_buffer("gripper_bounds", torch.tensor([amin[-1], amax[-1]], dtype=torch.float32))
        hi = torch.tensor(amax[:-1], dtype=torch.float32)
        lo = torch.tensor(amin[:-1], dtype=torch.float32)
        assert hi.shape[0] == self.out_features and lo.shape[0] == self.out_features
        self.register_buffer("action_max_bound", hi.view(1, 1, -1, 1) * self.ones)
        self.register_buffer("action_min_bound", lo.view(1, 1, -1, 1) * self.ones)
        self.gripper_fc = nn.Linear(hidden_size, 2)
        self.criterion = nn.CrossEntropyLoss()
        self.hidden_state = None

    def clear_hidden_state(self) -> None:
        self.hidden_state = None

    # ---- hot path ----------------------------------------------------------------------------------
    def fused_param_groups(self):
        """Parameters the native trainer lays out contiguously so that the four heads are ONE (184, H) matrix / (184,) bias in the
        arena (views, no per-step concat; their gradient lands in the same arena slice).  Order = the fused head layout."""
        H = self.prob_fc.weight.shape[1]
        rows, pad = self._head_rows()
        return [dict(attr="heads_w", params=[self.prob_fc.weight, self.mean_fc.weight, self.log_scale_fc.weight, self.gripper_fc.weight],
                     pad=pad * H, shape=(rows + pad, H)),
                dict(attr="heads_b", params=[self.prob_fc.bias, self.mean_fc.bias, self.log_scale_fc.bias, self.gripper_fc.bias], pad=pad,
                     shape=(rows + pad,))]

    def _head_rows(self):
        """(rows of the fused head matrix, zero rows appended so its width is a multiple of 8): 3 * out_features * n_dist + 2 gripper logits
        — 182 + 2 for the configured 6 x 10 (conf/model/action_decoder/logistic_decoder_rnn_calvin.yaml), derived, not assumed"""
        rows = 3 * self.out_features * self.n_dist + 2
        return rows, (-rows) % 8

    _fused = None      # {"heads_w": tensor view, "heads_b": tensor view} installed by ArenaTrainer

    def _heads(self, h: torch.Tensor) -> torch.Tensor:
        """(B,S,H) -> (B*S, 184): [logit_probs 60 | means 60 | log_scales 60 | gripper 2 | 2 zero pad columns]."""
        if self._fused is not None and (not torch.is_grad_enabled() or gradsink.get(self._fused["heads_w"]) is not None):
            # (the fused view carries no autograd edge: its gradient exists only as a sink — a trainer's, or the keeper's inside the step node)
            return HF.mlp(h.reshape(-1, h.shape[-1]), [(self._fused["heads_w"], self._fused["heads_b"], False)])
        pad = self._head_rows()[1]
        w = torch.cat([self.prob_fc.weight, self.mean_fc.weight, self.log_scale_fc.weight, self.gripper_fc.weight,
                       self.prob_fc.weight.new_zeros(pad, self.prob_fc.weight.shape[1])], dim=0)
        b = torch.cat([self.prob_fc.bias, self.mean_fc.bias, self.log_scale_fc.bias, self.gripper_fc.bias,
                       self.prob_fc.bias.new_zeros(pad)], dim=0)
        return HF.mlp(h.reshape(-1, h.shape[-1]), [(w, b, False)])

    def rnn_dropout(self, modality_scope=None) -> Tuple[float, int]:
        """(effective policy_rnn_dropout_p, RNG site) of a call: p only while the module trains; the stacked call (all modalities' rows in
        one tensor) has one site, a call per modality restarts its rows at 0 and takes the modality's own (vision_network.fc_site)"""
        return (self.policy_rnn_dropout_p if self.training else 0.0,
                fc_site(HF.DECODER_RNN_SITE, DECODER_RNN_MODALITY_SITES, modality_scope))

    def _rnn(self, latent_plan, perceptual_emb, latent_goal, time_major: bool = False, emb_tm: bool = False, modality_scope=None) -> torch.Tensor:
        r = self.rnn
        lo, hi = self.perceptual_emb_slice
        return HF.DecoderRNNFn.apply(latent_plan, perceptual_emb, latent_goal, lo, hi, r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0,
                                     r.bias_hh_l0, r.weight_ih_l1, r.weight_hh_l1, r.bias_ih_l1, r.bias_hh_l1, time_major, emb_tm,
                                     *self.rnn_dropout(modality_scope))

    def loss(self, latent_plan, perceptual_emb, latent_goal, actions, robot_obs, modality_scope=None) -> torch.Tensor:
        """modality_scope ("vis" / "lang", Hulc2.lmp_train; the training step itself calls loss_stacked / loss_segments): the modality this call
        serves — selects the RNN dropout's site"""
        return self.loss_stacked(latent_plan, perceptual_emb, latent_goal, [actions], [robot_obs], 1, modality_scope=modality_scope)[0]

    def loss_segments(self, plans, embs, goals, actions, robot_obs, scopes=None) -> torch.Tensor:
        """Decoder loss of several independent batches (the 'vis' and 'lang' modalities of one training step) in ONE
        pass over the recurrence: sequences are independent and the weights shared, so the batches are concatenated
        (64 rows per recurrent GEMM instead of 2 x 32 — half the launches of the latency-bound part) and the loss
        kernel returns one mean per segment, exactly what separate `loss` calls give (logistic_decoder_rnn.py:118-131).
        scopes: the modalities' names, for the separate passes of unequal batches (each draws its RNN dropout from its own site)."""
        n = len(plans)
        if n > 1 and len({p.shape[0] for p in plans}) > 1:          # unequal batches: fall back to separate passes
            return torch.cat([self.loss_stacked(plans[i], embs[i], goals[i], [actions[i]], [robot_obs[i]], 1,
                                                modality_scope=scopes[i] if scopes is not None else None) for i in range(n)])
        cat = (lambda ts: ts[0] if n == 1 else torch.cat(ts, dim=0))
        return self.loss_stacked(cat(plans), cat(embs), cat(goals), list(actions), list(robot_obs), n)

    def loss_stacked(self, plan, emb, goal, act, obs, n: int = 1, emb_tm: bool = False, modality_scope=None) -> torch.Tensor:
        """`loss_segments` on inputs that are already stacked on the batch axis (n equal segments, rows segment-major).
        emb_tm: `emb` is the decoder's embedding slice in time-major order (S, B, hi - lo), as EmbFanoutFn hands it over."""
        # training path: everything after the recurrence stays in the time-major row order the recurrent kernel leaves behind (row = step * B
        # + batch row): the heads read h1 in place, the loss maps rows to modality segments itself — no (B, S, 2048) transposes either way
        B, S = (emb.shape[1], emb.shape[0]) if emb_tm else (emb.shape[0], emb.shape[1])
        y = self._heads(self._rnn(plan, emb, goal, time_major=True, emb_tm=emb_tm, modality_scope=modality_scope))  # (S*B, heads)
        # targets in the same time-major row order, world -> tcp frame on the way (gripper_control.py:16-36): one launch for the stacked
        # modalities (act / obs: one tensor, or the list of per-modality tensors — no concatenation, no transposing copy)
        acts_l = list(act) if isinstance(act, (list, tuple)) else list(act.reshape(n, B // n, *act.shape[1:]).unbind(0))
        obs_l = list(obs) if isinstance(obs, (list, tuple)) else list(obs.reshape(n, B // n, *obs.shape[1:]).unbind(0))
        acts_t = HF.actions_time_major(acts_l, obs_l, self.gripper_control)           # (S * B, 7)
        lo_b, hi_b = self._bounds()
        return HF.MixLossFn.apply(y, acts_t, lo_b, hi_b, self.n_dist, self.num_classes,
                                  float(self.log_scale_min), float(self.gripper_alpha), n, B)

    def _bounds(self):
        """per-dimension action bounds as contiguous (A,) vectors (column 0 of the reference's (1, 1, A, n_mix) buffers), cached per buffer version"""
        key = (self.action_min_bound._version, self.action_max_bound._version, self.action_min_bound.data_ptr(), self.action_min_bound.device)
        c = self.__dict__.get("_bounds_cache")
        if c is None or c[0] != key:
            c = self.__dict__["_bounds_cache"] = (key, self.action_min_bound[0, 0, :, 0].contiguous(), self.action_max_bound[0, 0, :, 0].contiguous())
        return c[1], c[2]

    def forward(self, latent_plan, perceptual_emb, latent_goal, h_0: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """logistic_decoder_rnn.py:257-284 -> (logit_probs, log_scales, means, gripper_act, h_n).  With autograd enabled and no
        h_0 this is the training recurrence (h_n carries only layer 1's final state: the fused recurrence does not export layer 0);
        under torch.no_grad() or with a carried h_0 it is the inference sweep, which returns both final states."""
        y, h_n = self._head_outputs(latent_plan, perceptual_emb, latent_goal, h_0)
        return (*self._split_heads(y), h_n)

    def _head_outputs(self, latent_plan, perceptual_emb, latent_goal, h_0=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """fused head output y (B, S, 184) and h_n (2, B, H)"""
        B, S = perceptual_emb.shape[0], perceptual_emb.shape[1]
        if h_0 is not None or not torch.is_grad_enabled():
            r = self.rnn
            lo, hi = self.perceptual_emb_slice
            h, h_n = HF.decoder_rnn_infer(latent_plan, perceptual_emb, latent_goal, lo, hi, r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0,
                                          r.bias_hh_l0, r.weight_ih_l1, r.weight_hh_l1, r.bias_ih_l1, r.bias_hh_l1, h_0, *self.rnn_dropout())
        else:
            h = self._rnn(latent_plan, perceptual_emb, latent_goal)
            h_n = torch.stack([h.new_zeros(B, h.shape[-1]), h[:, -1]])
        return self._heads(h).reshape(B, S, -1), h_n

    def _split_heads(self, y: torch.Tensor):
        B, S = y.shape[0], y.shape[1]
        n = self.out_features * self.n_dist
        shp = (B, S, self.out_features, self.n_dist)
        logit_probs, means = y[..., :n].reshape(shp), y[..., n:2 * n].reshape(shp)
        log_scales = torch.clamp(y[..., 2 * n:3 * n], min=self.log_scale_min).reshape(shp)
        return logit_probs, log_scales, means, y[..., 3 * n:3 * n + 2]

    # ---- validation / rollout ----------------------------------------------------
    _sample_calls = 0

    def _sample(self, logit_probs, log_scales, means, gripper_act, u_mix=None, u_inv=None) -> torch.Tensor:
        """logistic_decoder_rnn.py:231-255 (Gumbel-max over the mixtures + logistic inverse CDF + gripper argmax) as one kernel.
        u_mix (B,S,A,n_mix) / u_inv (B,S,A): optional uniforms standing in for the reference's two torch.rand draws."""
        B, S, A, M = means.shape
        y = torch.cat([logit_probs.reshape(B * S, A * M), means.reshape(B * S, A * M), log_scales.reshape(B * S, A * M),
                       gripper_act.reshape(B * S, 2)], dim=1)
        return self._sample_heads(y, B, S, u_mix, u_inv)

    injected_uniforms: Optional[list] = None      # parity tests: [(u_mix, u_inv), ...] consumed one pair per _sample call

    def _sample_heads(self, y2d: torch.Tensor, B: int, S: int, u_mix=None, u_inv=None) -> torch.Tensor:
        if u_mix is None and self.injected_uniforms:
            u_mix, u_inv = self.injected_uniforms.pop(0)
        LogisticDecoderRNN._sample_calls += 1                     # a fresh counter-RNG stream per call
        seed = 0x5A3D1E00 + LogisticDecoderRNN._sample_calls
        A = self.out_features
        act = HF.mix_sample(y2d, A, self.n_dist, float(self.log_scale_min), self.gripper_bounds, seed,
                            None if u_mix is None else u_mix.reshape(B * S, A, self.n_dist),
                            None if u_inv is None else u_inv.reshape(B * S, A))
        return act.reshape(B, S, A + 1)

    @torch.no_grad()
    def act(self, latent_plan, perceptual_emb, latent_goal, robot_obs) -> torch.Tensor:
        """logistic_decoder_rnn.py:99-116: stateful decoding, the hidden state is carried across calls until clear_hidden_state()."""
        B, S = perceptual_emb.shape[0], perceptual_emb.shape[1]
        y, self.hidden_state = self._head_outputs(latent_plan, perceptual_emb, latent_goal,
                                                  self.hidden_state if self.hidden_state is not None else self._zero_state(B, perceptual_emb))
        pred = self._sample_heads(y.reshape(B * S, -1), B, S)
        return HF.tcp_to_world_frame(pred, robot_obs) if self.gripper_control else pred

    def _zero_state(self, B, like):
        return torch.zeros(2, B, self.rnn.hidden_size, dtype=torch.float32, device=like.device)

    @torch.no_grad()
    def loss_and_act(self, latent_plan, perceptual_emb, latent_goal, actions, robot_obs) -> Tuple[torch.Tensor, torch.Tensor]:
        """logistic_decoder_rnn.py:82-97: validation loss and one sampled action sequence from the same head outputs."""
        B, S = perceptual_emb.shape[0], perceptual_emb.shape[1]
        y, _ = self._head_outputs(latent_plan, perceptual_emb, latent_goal, None)
        y2d = y.reshape(B * S, -1)
        pred = self._sample_heads(y2d, B, S)
        acts = HF.world_to_tcp_frame(actions, robot_obs) if self.gripper_control else actions
        loss = HF.MixLossFn.apply(y2d, acts.reshape(-1, acts.shape[-1]), self.action_min_bound[0, 0, :, 0].contiguous(),
                                  self.action_max_bound[0, 0, :, 0].contiguous(), self.n_dist, self.num_classes,
                                  float(self.log_scale_min), float(self.gripper_alpha), 1)[0]
        return loss, (HF.tcp_to_world_frame(pred, robot_obs) if self.gripper_control else pred)
