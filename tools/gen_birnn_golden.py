"""Writes tests/golden/birnn/plan_recognition_birnn.npz: what the REFERENCE's PlanRecognitionBiRNNNetwork (imported through
oracle.gen_golden.import_reference(), float32 on the CPU, never edited) gives on the seeded case of tests/birnnref.module_case.

The fixture is data and holds no weights: parameters, input and cotangents are refilled from the seed by the yardstick (tests/birnnref.py),
as tests/normref.py does for its fixtures.  Contents: the state-dict key names and shapes; for B = 3, S = 5 the state logits, x and the
gradient of the input; every parameter gradient's L2 norm, the bias gradients whole and ROWS of the matrix gradients (a fixed sample: the
whole tensors would be 130 MB).  Runs only where the reference tree exists:   python tools/gen_birnn_golden.py"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle.gen_golden import import_reference  # noqa: E402
from tests import birnnref as R  # noqa: E402

SEED, B, S = 21, 3, 5
ROWS = (0, 1, 2, 517, 1000, 1023)                    # sampled rows of every matrix gradient (all of them exist in the smallest, 1024 x 4096)
OUT = ROOT / "tests" / "golden" / "birnn" / "plan_recognition_birnn.npz"


def main() -> None:
    ref = import_reference()
    torch.manual_seed(0)
    dist = ref["dist"].Distribution(dist="discrete", category_size=32, class_size=32)
    net = ref["prn"].PlanRecognitionBiRNNNetwork(in_features=128, plan_features=1024, action_space=7, birnn_dropout_p=0.0, dist=dist).float()
    params, emb, g_state, g_x = R.module_case(SEED, B, S)
    names = list(net.state_dict())
    assert names == list(params), "the reference's state dict and birnnref.module_shapes disagree"
    with torch.no_grad():
        for k, v in net.state_dict().items():
            assert tuple(v.shape) == tuple(params[k].shape), k
            v.copy_(params[k])
    e = emb.clone().requires_grad_(True)
    state, x = net(e)
    logits = state.logit.reshape(B, -1)
    (logits * g_state).sum().add((x * g_x).sum()).backward()
    out = {"names": np.array(names), "shapes": np.array([list(params[k].shape) + [0] * (2 - params[k].dim()) for k in names], dtype=np.int64),
           "rows": np.array(ROWS, dtype=np.int64), "case": np.array([SEED, B, S], dtype=np.int64),
           "logits": logits.detach().numpy(), "x": x.detach().numpy(), "g.emb": e.grad.numpy()}
    for k, p in net.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        out[f"norm.{k}"] = np.array(g.double().norm().item())
        out[f"g.{k}"] = (g[list(ROWS)] if g.dim() == 2 else g).numpy()
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size >> 10} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
