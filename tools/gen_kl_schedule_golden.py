#!/usr/bin/env python3
"""Record the reference's KL annealing values as tests/golden/kl_schedule.json.

    python tools/gen_kl_schedule_golden.py --reference /path/to/reference/checkout [--check]

Loads hulc2/utils/kl_callbacks.py of a reference checkout BY PATH (the package around it pulls in Lightning, Hydra, the simulator ...), with
a name-only stand-in for `pytorch_lightning` (Callback / LightningModule / Trainer are used as a base class and in annotations only), and
writes beta for epochs 0..60 of KLLinearSchedule and KLSigmoidSchedule under three parameter sets as float.hex() strings — recorded results
only, no code.  --check compares with the committed file instead of writing it.  tests/test_kl_schedule_cpu.py holds
hulc2_amd.kl_schedule to these values."""
import argparse
import importlib.util
import json
import sys
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "kl_schedule.json"
EPOCHS = 61
# (start_epoch, end_epoch, max_kl_beta): conf/callbacks/kl_schedule/{linear,sigmoid}.yaml with max_kl_beta = ${model.kl_beta} = 0.01
# (conf/model/default.yaml), then a ramp from epoch 0 and the shortest ramp there is
PARAMS = [(10, 50, 0.01), (0, 5, 1.0), (3, 4, 0.5)]


def load_reference(root: Path):
    path = root / "hulc2" / "utils" / "kl_callbacks.py"
    if not path.is_file():
        raise SystemExit(f"{path}: not found (--reference is the root of a reference checkout)")
    had = sys.modules.get("pytorch_lightning")
    stub = types.ModuleType("pytorch_lightning")
    for name in ("Callback", "LightningModule", "Trainer"):
        setattr(stub, name, type(name, (), {}))
    sys.modules["pytorch_lightning"] = stub
    try:
        spec = importlib.util.spec_from_file_location("_reference_kl_callbacks", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if had is None:
            del sys.modules["pytorch_lightning"]
        else:
            sys.modules["pytorch_lightning"] = had
    return mod


def record(mod) -> dict:
    sets = []
    for start, end, top in PARAMS:
        row = {"start_epoch": start, "end_epoch": end, "max_kl_beta": float(top).hex()}
        for key, cls in (("linear", mod.KLLinearSchedule), ("sigmoid", mod.KLSigmoidSchedule)):
            cb = cls(start, end, top)
            row[key] = [float(cb._anneal_fn(e)).hex() for e in range(EPOCHS)]
        sets.append(row)
    calls = []
    const = mod.KLConstantSchedule()
    probe = types.SimpleNamespace(current_epoch=0, set_kl_beta=calls.append)
    for e in range(EPOCHS):
        probe.current_epoch = e
        const.on_train_epoch_start(None, probe)
    return {"source": "hulc2/utils/kl_callbacks.py: KLLinearSchedule / KLSigmoidSchedule._anneal_fn(epoch), epoch = 0..60, as float.hex()",
            "epochs": EPOCHS,
            "constant": {"set_kl_beta_calls": len(calls),
                         "statement": "KLConstantSchedule.on_train_epoch_start never calls set_kl_beta: the model keeps its configured kl_beta"},
            "sets": sets}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, type=Path, help="root of a reference checkout (holds hulc2/utils/kl_callbacks.py)")
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    a = ap.parse_args()
    text = json.dumps(record(load_reference(a.reference)), indent=1) + "\n"
    if a.check:
        same = OUT.is_file() and OUT.read_text() == text
        print(f"{OUT.relative_to(ROOT)}: {'identical' if same else 'DIFFERS'}")
        return 0 if same else 1
    OUT.write_text(text)
    print(f"wrote {OUT.relative_to(ROOT)} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
