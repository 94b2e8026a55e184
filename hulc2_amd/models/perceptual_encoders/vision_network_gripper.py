"""Gripper-camera encoder (nature-CNN) on MI355X kernels.

Mirrors hulc2.models.perceptual_encoders.vision_network_gripper.VisionNetwork (reference
vision_network_gripper.py:11-26,57-89): keys conv_model.{0,2,4,7}, fc1.0, fc2, ln.  The reference's Flatten
runs over NCHW, so the NHWC conv output is re-ordered (a 3136-float copy per frame) before the first Linear.
"""
from typing import Tuple

import torch
import torch.nn as nn

from hulc2_amd import functional as HF
from hulc2_amd import kernels as kn
from hulc2_amd.models.perceptual_encoders.vision_network import GRIPPER_FC_MODALITY_SITES, GRIPPER_FC_SITE, check_dropout_p, fc_site


def nature_cnn(act_fn, num_c):
    return nn.Sequential(nn.Conv2d(num_c, 32, 8, stride=4), act_fn, nn.Conv2d(32, 64, 4, stride=2), act_fn,
                         nn.Conv2d(64, 64, 3, stride=1), act_fn, nn.Flatten(start_dim=1), nn.Linear(64 * 7 * 7, 128), act_fn)


class VisionNetwork(nn.Module):
    def __init__(self, input_width: int, input_height: int, conv_encoder: str, activation_function: str,
                 dropout_vis_fc: float, l2_normalize_output: bool, visual_features: int, num_c: int):
        super().__init__()
        if conv_encoder != "nature_cnn" or activation_function != "ReLU":
            raise NotImplementedError("hulc2_amd gripper VisionNetwork implements nature_cnn with ReLU; dropout_vis_fc in [0, 1) and "
                                      "l2_normalize_output are supported (conf/model/perceptual_encoder/rgb_gripper/default.yaml)")
        dropout_vis_fc = check_dropout_p(dropout_vis_fc, "dropout_vis_fc")
        self.l2_normalize_output = bool(l2_normalize_output)
        self.modality_scope = None           # set by ConcatEncoders in front of a per-modality call: selects the dropout site
        self.act_fn = nn.ReLU()
        self.conv_model = nature_cnn(self.act_fn, num_c)
        self.fc1 = nn.Sequential(nn.Linear(128, 512), self.act_fn, nn.Dropout(dropout_vis_fc))
        self.fc2 = nn.Linear(512, visual_features)
        self.ln = nn.LayerNorm(visual_features)

    def flatten_linears(self):
        """(weight, (C, H, W)) of Linear layers behind nn.Flatten: the trainer keeps their (h, w, c)-ordered bf16 shadows fresh"""
        return [(self.conv_model[7].weight, (64, 7, 7))]

    def lo_operands(self):
        """rounding remainders the split-operand forward of the fc1 -> fc2 head reads (precision site "encfc"; trainer-maintained)"""
        return [(self.fc1[0].weight, "lo"), (self.fc2.weight, "lo"), (self.conv_model[0].weight, "oihw_flat_lo")]

    def conv_params(self):
        c = self.conv_model
        return (c[0].weight, c[0].bias, c[2].weight, c[2].bias, c[4].weight, c[4].bias)

    def forward(self, x: torch.Tensor, aug_shift=None, aug_pad: int = 0, frame_index=None, pre_ln: bool = False) -> torch.Tensor:
        # (site "encfc": the exact-fp32 flatten-linear below gets the EXACT map — conv3 stores it next to the bf16 one, hulc_conv_desc.y_bf16)
        a3 = HF.conv_stack(x, self.conv_params(), grad_premasked=True, aug_pad=aug_pad, aug_shifts=aug_shift, frame_index=frame_index,
                           exact_out="encfc" in kn.fp32_sites())                                                                               # (N, 7, 7, 64) NHWC
        # nn.Flatten + Linear(3136, 128) + ReLU on the NHWC activation in place: the weight's columns are reordered, not the activations
        c = self.conv_model
        with kn.site_scope("encfc"):         # (selective precision)
            y = HF.flatten_linear_relu(a3, c[7].weight, c[7].bias)
            y = HF.mlp2_rows(y, self.fc1[0].weight, self.fc1[0].bias, self.fc2.weight, self.fc2.bias, drop_p=self.drop_p,
                             seed=fc_site(GRIPPER_FC_SITE, GRIPPER_FC_MODALITY_SITES, self.modality_scope))
        if pre_ln:
            return y
        return HF.layer_norm(y, self.ln.weight, self.ln.bias, self.ln.eps, l2=self.l2_normalize_output)

    @property
    def drop_p(self) -> float:
        """fc1's nn.Dropout is active iff the module is in training mode (nn.Dropout's rule)"""
        return float(self.fc1[2].p) if self.training else 0.0

    @staticmethod
    def calc_out_size(w: int, h: int, kernel_size: int, padding: int, stride: int) -> Tuple[int, int]:
        return (w - kernel_size + 2 * padding) // stride + 1, (h - kernel_size + 2 * padding) // stride + 1
