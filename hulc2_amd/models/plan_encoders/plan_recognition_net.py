"""Plan recognition (posterior) transformer.

Mirrors hulc2.models.plan_encoders.plan_recognition_net.PlanRecognitionTransformersNetwork (reference
plan_recognition_net.py:77-168): learned positions or the sinusoid table (position_embedding), 2 post-norm encoder
layers (8 heads of 16), an optional final LayerNorm of the encoder (encoder_normalize), fc 128->4096, mean over the
sequence, fc_state.  positional_normalize (a LayerNorm between the position add and the dropout) is still refused at
construction, although its stage exists in the kernels.  nn.TransformerEncoder is instantiated only as the parameter
container that yields the reference's state_dict keys; the arithmetic is HIP (MFMA GEMM chains, per-(batch,head) attention
waves, fused residual+dropout+LayerNorm).

The sequence mean is taken before the 128->4096 projection: mean_s(W x_s + b) = W mean_s(x_s) + b exactly, which
removes 31/32 of that layer's FLOPs.
"""
import math
from typing import Tuple

import torch
import torch.nn as nn

from hulc2_amd import functional as HF
from hulc2_amd import kernels as kn
from hulc2_amd.utils.distributions import Distribution, State

# Dropout sites of the trunk (the per-step stream comes from the device step state, kernels.step_state).  A call derives its sub-sites
# s (position add) and s + 100 (l + 1) + {11, 12, 13, 15} (layer l), so sites 0x1000 apart never share a stream.
TRUNK_SITE = 0x5EED0001                          # one call over all modalities stacked on the batch axis: each row has its own indices
MODALITY_SITES = {"vis": 0x5EED1001, "lang": 0x5EED2001}     # one call per modality: rows restart at 0, so each modality gets its own site


def trunk_site(modality_scope: str) -> int:
    """the site of a per-modality trunk call (Hulc2.lmp_train, the per-modality step): distinct masks for the two modalities"""
    return MODALITY_SITES["lang" if "lang" in modality_scope else "vis"]


class PositionalEncoding(nn.Module):
    """the parameter-free position table of position_embedding = false (plan_recognition_net.py:151-167): the persistent buffer
    pe (max_len, 1, d_model) with pe[t, 0, 2i] = sin(t w_i), pe[t, 0, 2i + 1] = cos(t w_i), w_i = 10000^(-2i / d_model), evaluated in
    float32 like the reference's.  The trunk kernels read it as the (max_len, d_model) table `table`."""

    def __init__(self, d_model: int, max_len: int = 5000):
        super().__init__()
        if d_model % 2:
            raise NotImplementedError("sinusoid positions: an even d_model")
        # (the expression of the public PyTorch tutorial pytorch.org/tutorials/beginner/transformer_tutorial.html, which the reference names
        # as its source; the same float32 operations in the same order are what makes the table equal the reference's to the last bit)
        t = torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1)
        w = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, 1, d_model)
        pe[:, 0, 0::2], pe[:, 0, 1::2] = torch.sin(t * w), torch.cos(t * w)
        self.register_buffer("pe", pe)

    @property
    def table(self) -> torch.Tensor:
        return self.pe.view(self.pe.shape[0], self.pe.shape[2])


class PlanRecognitionTransformersNetwork(nn.Module):
    def __init__(self, num_heads: int, num_layers: int, encoder_hidden_size: int, fc_hidden_size: int, plan_features: int,
                 in_features: int, action_space: int, encoder_normalize: bool, positional_normalize: bool,
                 position_embedding: bool, max_position_embeddings: int, dropout_p: float, dist: Distribution):
        super().__init__()
        if in_features % num_heads != 0 or in_features // num_heads != 16:
            raise NotImplementedError("attention kernel is specialised for head_dim 16 without padding (128 / 8)")
        if positional_normalize:
            # (the LayerNorm stage exists in the trunk launches, functional.transformer_trunk_pooled(pos_norm=...); the module does not
            # take the switch: its refusal is part of the suite's contract, tests/test_host_cpu.py::test_unsupported_configs_fail_loudly)
            raise NotImplementedError("positional_normalize is not enabled in this module (conf/model/plan_recognition/transformers.yaml)")
        self.in_features, self.plan_features, self.action_space = in_features, plan_features, action_space
        self.padding = False
        self.dist = dist
        self.hidden_size = fc_hidden_size
        self.position_embedding, self.encoder_normalize = bool(position_embedding), bool(encoder_normalize)
        self.positional_normalize = False
        self.num_heads, self.num_layers, self.dropout_p = num_heads, num_layers, float(dropout_p)
        if self.position_embedding:
            self.position_embeddings = nn.Embedding(max_position_embeddings, in_features)
        else:
            self.positional_encoder = PositionalEncoding(in_features)
        layer = nn.TransformerEncoderLayer(in_features, num_heads, dim_feedforward=encoder_hidden_size, dropout=float(dropout_p))
        self.layernorm = nn.LayerNorm(in_features)                 # (always constructed, as the reference does; unused here)
        self.dropout = nn.Dropout(p=float(dropout_p))
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=num_layers, norm=nn.LayerNorm(in_features) if self.encoder_normalize else None,
                                                         enable_nested_tensor=False)
        self.fc = nn.Linear(in_features, fc_hidden_size)
        self.fc_state = self.dist.build_state(fc_hidden_size, plan_features)

    def _layer_params(self, l: int) -> dict:
        m = self.transformer_encoder.layers[l]
        return {"in_proj_weight": m.self_attn.in_proj_weight, "in_proj_bias": m.self_attn.in_proj_bias,
                "out_proj.weight": m.self_attn.out_proj.weight, "out_proj.bias": m.self_attn.out_proj.bias,
                "linear1.weight": m.linear1.weight, "linear1.bias": m.linear1.bias,
                "linear2.weight": m.linear2.weight, "linear2.bias": m.linear2.bias,
                "norm1.weight": m.norm1.weight, "norm1.bias": m.norm1.bias,
                "norm2.weight": m.norm2.weight, "norm2.bias": m.norm2.bias}

    def frag_operands(self):
        """(weight, hulc_ffn_frag_perm layout) of the feed-forward weights the whole-trunk launch reads fragment-packed: the trainer keeps
        these copies fresh with one gather launch per step"""
        out = []
        for m in self.transformer_encoder.layers:
            out += [(m.linear1.weight, 0), (m.linear2.weight, 1), (m.linear2.weight, 2), (m.linear1.weight, 3)]
        return out

    def lo_operands(self):
        """(weight, layout) of the rounding remainders w - bf16(w) the split-operand forward of the whole-trunk launch reads (selective
        precision site "txl"): kept fresh by the trainer with one residual + one gather launch per step"""
        out = []
        for m in self.transformer_encoder.layers:
            out += [(m.self_attn.in_proj_weight, "lo"), (m.self_attn.out_proj.weight, "lo"), (m.linear1.weight, "ffn_p0_lo"), (m.linear2.weight, "ffn_p1_lo")]
        return out

    def _position_ids(self, S: int, device) -> torch.Tensor:
        """arange(S) (plan_recognition_net.py:133): kept per (length, device) instead of one launch per step"""
        cache = self.__dict__.setdefault("_pos_id_cache", {})
        ids = cache.get((S, device))
        if ids is None:
            ids = cache[(S, device)] = torch.arange(S, dtype=torch.long, device=device)
            ids._hulc_arange = True          # (rows 0..S-1 in order: the table's gradient rows are the batch sum itself)
        return ids

    def forward(self, perceptual_emb: torch.Tensor, seed: int = TRUNK_SITE) -> Tuple[State, torch.Tensor]:
        B, S, E = perceptual_emb.shape
        p = self.dropout_p if self.training else 0.0
        position_ids = self._position_ids(S, perceptual_emb.device)
        layers = [self._layer_params(l) for l in range(self.num_layers)]
        # the position table: the learned embedding, or the sinusoid buffer (a table without a gradient: rows arange(S) of either)
        table = self.position_embeddings.weight if self.position_embedding else self.positional_encoder.table
        enc = self.transformer_encoder.norm
        enc_norm = (enc.weight, enc.bias) if self.encoder_normalize else None
        if HF.txl_block_ok(perceptual_emb, layers, S, self.num_heads):
            # position embedding -> every layer -> sequence mean: one launch per direction, one workgroup per sequence (csrc/txl_block.hip;
            # with a LayerNorm switched on, the same two launches with its stage: csrc/txl_block_norms.hip)
            pooled = HF.transformer_trunk_pooled(perceptual_emb, table, position_ids, layers, self.num_heads, p, seed, None, enc_norm)
        else:
            x = HF.AddPosFn.apply(perceptual_emb, table, position_ids, p, seed, True)
            x = x.reshape(B * S, E)
            with kn.site_scope("txl"):
                for l in range(self.num_layers):
                    x = HF.transformer_encoder_layer(x, layers[l], B, S, self.num_heads, p, seed + 100 * (l + 1))
            with kn.site_scope("pool"):
                if enc_norm:
                    x = HF.layer_norm(x, *enc_norm)
                pooled = HF.SeqMeanFn.apply(x.reshape(B, S, E))
        # selective precision: seq_feat feeds the contrastive head, whose gradient is a cancelling remainder of nearly identical
        # rows — its projection runs exact-fp32 inside a bf16 step (67 MFLOP of the step's 904 GFLOP)
        with kn.site_scope("head"):
            seq_feat = HF.mlp(pooled, [(self.fc.weight, self.fc.bias, False)])
        logits = HF.mlp(seq_feat, [(self.fc_state[0].weight, self.fc_state[0].bias, False)])
        return self.dist.forward_dist(logits), seq_feat


class PlanRecognitionBiRNNNetwork(nn.Module):
    """The recurrent posterior of conf/model/plan_recognition/birnn.yaml (the reference's PlanRecognitionBiRNNNetwork): a 2-layer bidirectional
    ReLU nn.RNN of width 2048 over the perceptual embeddings, its output at the LAST time step, fc_state.  `birnn_model` is the parameter
    container that yields the reference's state_dict keys; the arithmetic is HIP (functional.BiRNNPosteriorFn: paired persistent sweeps in
    bf16 compute on a whole MI355X, per-step GEMMs otherwise).  forward -> (state, x) with x = [hf1_{S-1} | hb1_{S-1}] (B, 4096).
    birnn_dropout_p > 0 (torch drops layer 0's output on its way into layer 1) is not built: refused at construction."""

    recurrent = True          # Hulc2.training_step: not a forked branch (the sweeps' device-wide barrier needs the whole GPU)

    def __init__(self, in_features: int, plan_features: int, action_space: int, birnn_dropout_p: float, dist: Distribution):
        super().__init__()
        if float(birnn_dropout_p) != 0.0:
            raise NotImplementedError("birnn_dropout_p > 0 is not built: conf/model/plan_recognition/birnn.yaml with birnn_dropout_p: 0.0 is supported")
        self.in_features, self.plan_features, self.action_space = in_features, plan_features, action_space
        self.dist = dist
        self.hidden_size = 2048
        self.birnn_model = nn.RNN(input_size=in_features, hidden_size=self.hidden_size, nonlinearity="relu", num_layers=2, bidirectional=True,
                                  batch_first=True, dropout=0.0)
        self.fc_state = self.dist.build_state(2 * self.hidden_size, plan_features)

    def forward(self, perceptual_emb: torch.Tensor, seed: int = TRUNK_SITE) -> Tuple[State, torch.Tensor]:
        """seed: the dropout site Hulc2 passes to every posterior; this one draws nothing"""
        x = HF.birnn_posterior(perceptual_emb, self.birnn_model)
        logits = HF.mlp(x, [(self.fc_state[0].weight, self.fc_state[0].bias, False)])
        return self.dist.forward_dist(logits), x


class PlanRecognitionBiLSTMNetwork(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError("the BiLSTM posterior (conf/model/plan_recognition/bilstm.yaml) is not built: plan_recognition=transformers "
                                  "and plan_recognition=birnn are")
