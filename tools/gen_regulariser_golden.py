#!/usr/bin/env python3
"""Record the reference's encoders with their regularisers on as tests/golden/regularisers/encoder_regularisers.npz.

    python tools/gen_regulariser_golden.py --reference /path/to/reference/checkout [--check]

Imports the reference's two VisionNetworks and two goal encoders in place (oracle.gen_golden.import_reference), instantiates them in float64
train mode with dropout_vis_fc = 0.1, word_dropout_p = 0.1 and every l2_normalize flag set, and loads the seeded parameters of
hulc2_amd.synthetic.  torch.nn.functional.dropout is replaced by a call-order replay (tests/test_dropout_reference_cpu._replaying_dropout)
whose keep-scales are the counter RNG's (oracle/counter_rng.py) under this project's sites and element indices (tests/regref.py), so the
fixture pins WHERE the reference drops and normalises, on the masks the kernels draw.  Recorded per module: the output, the gradient of
(output * r).sum() with respect to the input (the cameras': every 8th pixel) and to three or four parameters — results only, no code.
--check compares with the committed file instead of writing it.  tests/test_encoder_regularisers_cpu.py holds tests/regref.py to these
values, tests/test_encoder_regularisers_gpu.py the modules."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "tests" / "golden" / "regularisers" / "encoder_regularisers.npz"      # (a directory of its own: oracle/gen_golden.py --check owns the *.npz files directly under tests/golden)


def build(refmods, tag):
    from tests import regref as G
    if tag == "static":
        return refmods["vn"].VisionNetwork(input_width=200, input_height=200, activation_function="ReLU", dropout_vis_fc=G.P,
                                           l2_normalize_output=True, visual_features=64, num_c=3, use_sinusoid=False, spatial_softmax_temp=1.0)
    if tag == "gripper":
        return refmods["vng"].VisionNetwork(input_width=84, input_height=84, conv_encoder="nature_cnn", activation_function="ReLU",
                                            dropout_vis_fc=G.P, l2_normalize_output=True, visual_features=64, num_c=3)
    if tag == "visual_goal":
        return refmods["goal"].VisualGoalEncoder(hidden_size=2048, latent_goal_features=32, in_features=128, l2_normalize_goal_embeddings=True,
                                                 activation_function="ReLU")
    return refmods["goal"].LanguageGoalEncoder(lang_net=None, in_features=384, hidden_size=2048, latent_goal_features=32,
                                               l2_normalize_goal_embeddings=True, word_dropout_p=G.P, activation_function="ReLU")


def record(reference: Path) -> dict:
    import torch.nn.functional as F

    from hulc2_amd import synthetic as syn
    from oracle import gen_golden
    from tests import regref as G
    from tests.test_dropout_reference_cpu import _replaying_dropout

    if not (reference / "hulc2" / "models" / "encoders" / "goal_encoders.py").is_file():
        raise SystemExit(f"{reference}: not the root of a reference checkout")
    gen_golden.REF = reference
    refmods = gen_golden.import_reference()
    arrays = {"seed": np.int64(G.SEED), "p": np.float64(G.P), "word": np.uint64(G.WORD)}
    torch.set_num_threads(min(8, torch.get_num_threads()))
    for tag, (prefix, _shape, _kind, _width) in G.MODULES.items():
        mod = build(refmods, tag)
        flat = {prefix + k: v for k, v in mod.state_dict().items()}
        syn.fill_state_dict_(flat, G.SEED)                     # in place, float32 recipe; then widened exactly
        mod = mod.double().train()
        x, r = G.inputs(tag)
        x.requires_grad_(True)
        keep = G.mask_of(tag, x.shape[0])
        replay, queue = _replaying_dropout([keep] if keep is not None else [], G.P)
        real = F.dropout
        F.dropout = replay
        try:
            y = mod(x)
        finally:
            F.dropout = real
        assert not queue, f"{tag}: the reference called dropout {len(queue)} time(s) fewer than expected"
        named = dict(mod.named_parameters())
        names = [n for n, _ in G.GRAD_PARAMS[tag]]
        grads = torch.autograd.grad((y * r).sum(), [x] + [named[n] for n in names])
        arrays.update(G.record(tag, y, grads[0], dict(zip(names, grads[1:]))))
    return arrays


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, type=Path, help="root of a reference checkout (holds hulc2/models/...)")
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    a = ap.parse_args()
    arrays = record(a.reference)
    if a.check:
        same = OUT.is_file()
        if same:
            have = dict(np.load(OUT, allow_pickle=False))
            # float64 sums in another thread partition move the last bits: equal to 1e-12 of each array's largest magnitude
            same = set(have) == set(arrays) and all(
                have[k].shape == np.shape(arrays[k])
                and float(np.max(np.abs(have[k].astype(np.float64) - np.asarray(arrays[k], dtype=np.float64)), initial=0.0))
                <= 1e-12 * max(float(np.max(np.abs(have[k].astype(np.float64)), initial=0.0)), 1e-300) for k in arrays)
        print(f"{OUT.relative_to(ROOT)}: {'identical' if same else 'DIFFERS'}")
        return 0 if same else 1
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT.relative_to(ROOT)} ({OUT.stat().st_size} bytes, {len(arrays)} arrays)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
