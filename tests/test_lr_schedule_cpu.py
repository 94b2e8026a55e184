"""The configured `lr_scheduler` reaches the optimizer (reference: hulc2/models/hulc2.py:160-198, conf/model/lr_scheduler/*.yaml) — host side:
`Hulc2.configure_optimizers` instantiates the configured transformers schedule after `compute_warmup`, and `optim.lr_lambda_from_config`
hands the same factor function to the native trainer.  Checked against the transformers functions themselves, value for value."""
import sys
import types
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from hulc2_amd.compat import Config, instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402

# the three configs the reference ships under conf/model/lr_scheduler/, written out
CONFIGS = {
    "constant": {"_target_": "transformers.get_constant_schedule"},
    "linear": {"_target_": "transformers.get_linear_schedule_with_warmup", "num_training_steps": -1, "num_warmup_steps": 0.1},
    "cosine": {"_target_": "transformers.get_cosine_schedule_with_warmup", "num_training_steps": -1, "num_warmup_steps": 0.1,
               "num_cycles": 0.5},
}
TOTAL, WARMUP, STEPS = 200, 20, 40


def _direct(name, optimizer):
    """the same transformers function built directly, with the numbers compute_warmup must arrive at"""
    import transformers
    if name == "constant":
        return transformers.get_constant_schedule(optimizer)
    if name == "linear":
        return transformers.get_linear_schedule_with_warmup(optimizer, num_warmup_steps=WARMUP, num_training_steps=TOTAL)
    return transformers.get_cosine_schedule_with_warmup(optimizer, num_warmup_steps=WARMUP, num_training_steps=TOTAL, num_cycles=0.5)


def _lr_sequence(opt, sched):
    out = [opt.param_groups[0]["lr"]]
    for _ in range(STEPS):
        opt.step()
        sched.step()
        out.append(opt.param_groups[0]["lr"])
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_configure_optimizers_follows_the_configured_schedule(name, monkeypatch):
    """40 steps of optimizer + scheduler from `configure_optimizers()`: the learning rates are the transformers function's own, as Python floats.
    (Before the scheduler was honoured every value was 2e-4: the linear and cosine cases failed, the constant case is the control.)"""
    ref_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=2e-4)
    want = _lr_sequence(ref_opt, _direct(name, ref_opt))
    if name != "constant":
        assert want[0] == 0.0 and want[WARMUP] == 2e-4 and want[STEPS] < 2e-4, "the direct schedule itself must warm up and decay"
    cfg = default_model_config()
    cfg["lr_scheduler"] = Config.wrap(dict(CONFIGS[name]))
    m = instantiate(cfg)
    m.trainer = types.SimpleNamespace(estimated_stepping_batches=TOTAL)
    for torch_adam in ("1", None):                             # torch.optim.Adam itself, and the drop-in subclass (torch's step on the CPU)
        if torch_adam:
            monkeypatch.setenv("HULC_TORCH_ADAM", torch_adam)
        else:
            monkeypatch.delenv("HULC_TORCH_ADAM", raising=False)
        m.lr_scheduler = Config.wrap(dict(CONFIGS[name]))
        out = m.configure_optimizers()
        assert set(out) == {"optimizer", "lr_scheduler"}
        assert {k: v for k, v in out["lr_scheduler"].items() if k != "scheduler"} == {"interval": "step", "frequency": 1}
        opt = out["optimizer"]
        assert isinstance(opt, torch.optim.Adam) and (type(opt) is torch.optim.Adam) == bool(torch_adam)
        got = _lr_sequence(opt, out["lr_scheduler"]["scheduler"])
        assert got == want, (name, torch_adam, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:5])
        if name != "constant":
            assert m.lr_scheduler["num_training_steps"] == TOTAL and m.lr_scheduler["num_warmup_steps"] == WARMUP


def test_compute_warmup():
    """hulc2.py:164-183: negative steps are inferred from the trainer, a float warm-up is a fraction, the result is cut to an int"""
    from hulc2_amd.models.hulc2 import Hulc2
    m = Hulc2.__new__(Hulc2)                                   # (the two methods read nothing but self.trainer)
    torch.nn.Module.__init__(m)
    object.__setattr__(m, "trainer", types.SimpleNamespace(estimated_stepping_batches=200))
    assert m.num_training_steps == 200 and isinstance(m.num_training_steps, int)
    assert m.compute_warmup(-1, 0.1) == (200, 20)
    assert m.compute_warmup(1000, 50) == (1000, 50)
    assert m.compute_warmup(1000, 0.25) == (1000, 250)
    assert all(isinstance(x, int) for x in m.compute_warmup(-1, 0.1))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_schedule_helper_hands_out_the_schedulers_own_function(name):
    from hulc2_amd.optim import lr_lambda_from_config
    f = lr_lambda_from_config(CONFIGS[name], num_training_steps=TOTAL)
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=2e-4)
    g = _direct(name, opt).lr_lambdas[0]
    assert [f(k) for k in range(STEPS)] == [g(k) for k in range(STEPS)]
    assert CONFIGS[name].get("num_training_steps", -1) == -1   # the caller's config is left as it was


def test_unknown_schedule_target_raises_by_name():
    """no silent constant: a target that cannot be imported raises and the message names it — from the helper and from the model's hook"""
    from hulc2_amd.optim import lr_lambda_from_config, make_lr_scheduler
    bad = {"_target_": "no_such_scheduler_package.get_schedule", "num_training_steps": -1, "num_warmup_steps": 0.1}
    with pytest.raises(ImportError, match="no_such_scheduler_package.get_schedule"):
        lr_lambda_from_config(bad, num_training_steps=TOTAL)
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=2e-4)
    with pytest.raises(ImportError, match="no_such_scheduler_package.get_schedule"):
        make_lr_scheduler({"_target_": "no_such_scheduler_package.get_schedule"}, opt)


def test_constant_schedule_has_a_stand_in_without_transformers(monkeypatch):
    """without an importable `transformers` the constant target keeps its factor of 1.0; the warm-up targets raise by name"""
    from hulc2_amd.optim import make_lr_scheduler
    monkeypatch.setitem(sys.modules, "transformers", None)     # `import transformers` now raises ImportError
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=2e-4)
    sched = make_lr_scheduler(CONFIGS["constant"], opt)
    assert _lr_sequence(opt, sched) == [2e-4] * (STEPS + 1)
    with pytest.raises(ImportError, match="transformers.get_linear_schedule_with_warmup"):
        make_lr_scheduler({**CONFIGS["linear"], "num_training_steps": TOTAL, "num_warmup_steps": WARMUP}, opt)


def test_trainer_schedule_bookkeeping_on_the_host():
    """ArenaTrainer.set_lr_schedule / state_dict / torch interchange without a launch: base rate and position travel with the checkpoint,
    `initial_lr` appears in the torch group only when a schedule is attached"""
    from hulc2_amd.optim import lr_lambda_from_config
    from hulc2_amd.trainer import ArenaTrainer
    f = lr_lambda_from_config(CONFIGS["linear"], num_training_steps=TOTAL)
    net = lambda: torch.nn.Sequential(torch.nn.Linear(6, 9), torch.nn.ReLU(), torch.nn.Linear(9, 2))  # noqa: E731
    tr = ArenaTrainer(net())
    plain = tr.to_torch_adam_state_dict()["param_groups"][0]
    assert "initial_lr" not in plain and plain["lr"] == 2e-4 and tr._lr_dev is None
    tr.set_lr_schedule(f)
    assert tr.lr == 0.0 and float(tr._lr_dev) == 0.0
    tr._opt_steps = 7                                          # (as after seven optimizer steps)
    sd = tr.state_dict()
    assert sd["lr_schedule"] == {"base_lr": 2e-4, "position": 7, "device_lr": True}
    g = tr.to_torch_adam_state_dict()["param_groups"][0]
    assert g["initial_lr"] == 2e-4 and g["lr"] == 2e-4 * f(7)
    tr2 = ArenaTrainer(net(), lr=1.0)
    tr2.load_state_dict(sd)
    tr2.set_lr_schedule(f)
    assert tr2.base_lr == 2e-4 and tr2._opt_steps == 7 and tr2.lr == 2e-4 * f(7)
    import ctypes
    assert float(tr2._lr_dev) == ctypes.c_float(2e-4 * f(7)).value
    tr3 = ArenaTrainer(net(), lr=1.0)
    tr3.from_torch_adam_state_dict({"state": {}, "param_groups": [dict(g)]})
    assert tr3.base_lr == 2e-4 and tr3.lr == g["lr"]
