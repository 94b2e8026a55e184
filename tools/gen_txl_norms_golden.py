"""Generate tests/golden/txl_norms/plan_recognition_norms.npz: the REFERENCE's PlanRecognitionTransformersNetwork on the CPU (fp32) for all
eight combinations of encoder_normalize / positional_normalize / position_embedding (conf/model/plan_recognition/transformers.yaml).

usage: python tools/gen_txl_norms_golden.py /path/to/the/reference/checkout

Runs only where the reference exists; the tests read the fixture alone.  The reference's modules are imported in place, the way
oracle/gen_golden.py imports them; nothing of their text is copied.  The fixture holds no weights: parameters, input and cotangents are a
pure function of seeds (tests/normref.py fill_state_dict_ / fixture_inputs), and the tests fill their module the same way.  Per combination
(prefix = normref.combo_tag, e.g. "nny/" for the yaml's defaults): the sorted state-dict names and shapes, logits, seq_feat, the input
gradient for the fixed cotangents, the gradients of layernorm.*, transformer_encoder.norm.* and position_embeddings.weight where they
exist, and pe[:32, 0] in sinusoid mode.  The directory is this fixture's own: oracle/gen_golden.py --check keeps owning tests/golden/*.npz."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import gen_golden  # noqa: E402
from tests import normref as N  # noqa: E402

GRADS = ("layernorm.weight", "layernorm.bias", "transformer_encoder.norm.weight", "transformer_encoder.norm.bias", "position_embeddings.weight")


def main(ref: str) -> None:
    gen_golden.REF = Path(ref)
    R = gen_golden.import_reference()
    torch.manual_seed(0)
    torch.set_num_threads(1)
    emb0, c_logits, c_feat = N.fixture_inputs()
    out = {}
    for combo in N.COMBOS:
        tag = N.combo_tag(combo) + "/"
        net = R["prn"].PlanRecognitionTransformersNetwork(**N.MODULE_KW, **dict(zip(N.SWITCHES, combo)), dist=R["dist"].Distribution(**N.DIST_KW))
        net.eval()                                                   # (dropout_p is 0: eval only selects the plain attention path)
        sd = net.state_dict()
        N.fill_state_dict_(sd)
        names = sorted(sd)
        out[tag + "names"] = np.array(names)
        out[tag + "shapes"] = np.array([",".join(str(int(v)) for v in sd[k].shape) for k in names])
        emb = emb0.clone().requires_grad_(True)
        state, seq_feat = net(emb)
        logits = state.logit.reshape(N.FIX_B, -1)
        ((logits * c_logits).sum() + (seq_feat * c_feat).sum()).backward()
        out[tag + "logits"], out[tag + "seq_feat"] = logits.detach().numpy(), seq_feat.detach().numpy()
        out[tag + "d_emb"] = emb.grad.numpy()
        params = dict(net.named_parameters())
        for k in GRADS:
            if k in params and params[k].grad is not None:
                out[tag + "grad/" + k] = params[k].grad.numpy()
        if not combo[2]:
            out[tag + "pe32"] = sd["positional_encoder.pe"][:32, 0].numpy()
    dst = ROOT / N.GOLDEN
    dst.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(dst, **out)
    print(f"[gen_txl_norms_golden] {dst} ({dst.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
