"""Gradient accumulation (ArenaTrainer(accumulate_grad_batches=k)), the parts that need no GPU: the header and the exported symbol, the
argument checks, the accumulator's allocation, the window's place in state_dict() / load_state_dict()."""
import copy
import ctypes as c
import re
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from hulc2_amd import kernels as kn, lib as L  # noqa: E402
from hulc2_amd.trainer import ArenaTrainer  # noqa: E402


def _trainer(**kw):
    torch.manual_seed(0)
    return ArenaTrainer(torch.nn.Linear(8, 8), **kw)


# ---- the header and the library ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbol():
    text = (ROOT / "include" / "hulc2_amd.h").read_text()
    flat = " ".join(text.split())
    assert "int hulc_grad_accumulate(float* acc, float* g, long n, int mode, float scale, void* stream);" in flat
    protos = L.parse_prototypes(text)
    assert protos["hulc_grad_accumulate"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_long, c.c_int, c.c_float, c.c_void_p])
    so = L.load()
    assert so.hulc_abi_version() == 7
    fn = so.hulc_grad_accumulate                                   # (AttributeError if the library does not export it)
    assert fn.restype is c.c_int and list(fn.argtypes) == protos["hulc_grad_accumulate"][1]


def test_header_states_the_modes_and_the_order_of_the_two_roundings():
    text = (ROOT / "include" / "hulc2_amd.h").read_text()
    doc = text[text.index("GRADIENT ACCUMULATION"):text.index("int hulc_grad_accumulate(")]
    for mode in (r"mode 0 \(store\)\s+acc\[i\] = g\[i\]", r"mode 1 \(add\)\s+acc\[i\] = fl\(acc\[i\] \+ g\[i\]\)",
                 r"mode 2 \(finish\)\s+g\[i\]\s+= fl\(fl\(acc\[i\] \+ g\[i\]\) \* scale\)"):
        assert re.search(mode, doc), mode
    assert re.search(r"add FIRST, rounded to fp32, and THEN the multiply, rounded to fp32", doc)
    assert re.search(r"never contracted", doc) and re.search(r"captured", doc)


def test_host_side_refusals_need_no_device():
    """the entry point checks its arguments before it touches the device: the codes of the header, through the library itself"""
    so = L.load()
    buf = (c.c_float * 64)()
    base = c.addressof(buf)
    a, g = (base + 15) // 16 * 16, (base + 15) // 16 * 16 + 64
    assert so.hulc_grad_accumulate(None, None, 0, 0, 1.0, None) == 0, "n == 0 is a successful no-op, whatever the pointers"
    assert so.hulc_grad_accumulate(None, g, 4, 0, 1.0, None) == -1 and so.hulc_grad_accumulate(a, None, 4, 1, 1.0, None) == -1
    assert so.hulc_grad_accumulate(a, g, -1, 0, 1.0, None) == -2
    for mode in (-1, 3):
        assert so.hulc_grad_accumulate(a, g, 4, mode, 1.0, None) == -2
    assert so.hulc_grad_accumulate(a, a + 16, 8, 1, 1.0, None) == -2, "overlapping ranges"
    assert so.hulc_grad_accumulate(a, a, 4, 2, 1.0, None) == -2
    assert so.hulc_grad_accumulate(a + 4, g, 4, 0, 1.0, None) == -4 and so.hulc_grad_accumulate(a, g + 4, 4, 0, 1.0, None) == -4
    assert b"hulc_grad_accumulate" in so.hulc_last_error()


def test_binding_refuses_cpu_tensors_and_unknown_modes():
    x, y = torch.zeros(8), torch.zeros(8)
    with pytest.raises(L.HulcKernelError):
        kn.grad_accumulate(x, y, 8, "store")
    for mode in (3, "sum", None):
        with pytest.raises(L.HulcKernelError):
            kn.grad_accumulate(x, y, 8, mode)


# ---- the constructor ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, -1, 1.5, True, "2"])
def test_trainer_refuses_anything_but_an_int_from_one(bad):
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        _trainer(accumulate_grad_batches=bad)


def test_accumulator_exists_only_for_a_window_longer_than_one():
    tr = _trainer(accumulate_grad_batches=1)
    assert tr.flat_acc is None and tr.accumulate_grad_batches == 1 and tr.micro_batch == 0
    tr.close()
    assert _trainer().flat_acc is None
    tr = _trainer(accumulate_grad_batches=3)
    try:
        assert tr.accumulate_grad_batches == 3 and tr.micro_batch == 0
        assert tr.flat_acc.shape == (tr.total,) and tr.flat_acc.dtype == torch.float32 and tr.flat_acc.device == tr.flat_g.device
        assert tr.flat_acc.data_ptr() != tr.flat_g.data_ptr()
    finally:
        tr.close()


def test_set_accumulate_grad_batches():
    tr = _trainer(accumulate_grad_batches=2)
    try:
        tr.graph_fb = tr.graph_enc = tr.graph_opt = object()          # stand-ins for captured graphs
        tr.set_accumulate_grad_batches(2)                              # nothing changed: they stay
        assert tr.graph_opt is not None
        tr.set_accumulate_grad_batches(4)
        assert tr.graph_fb is None and tr.graph_opt is None and tr.accumulate_grad_batches == 4 and tr.flat_acc.numel() == tr.total
        tr.set_accumulate_grad_batches(1)
        assert tr.flat_acc is None
        for bad in (0, True, 2.0):
            with pytest.raises(ValueError):
                tr.set_accumulate_grad_batches(bad)
        tr.set_accumulate_grad_batches(3)
        tr.micro_batch = 1                                             # an open window
        with pytest.raises(RuntimeError, match="window boundary"):
            tr.set_accumulate_grad_batches(2)
        assert tr.accumulate_grad_batches == 3
    finally:
        tr.close()


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------------------------
def test_window_round_trips_at_a_boundary():
    tr = _trainer(accumulate_grad_batches=3)
    sd = copy.deepcopy(tr.state_dict())
    assert sd["accumulate"] == {"k": 3, "position": 0}
    tr.close()
    tr2 = _trainer(accumulate_grad_batches=3)
    tr2.micro_batch = 2
    tr2.load_state_dict(sd)
    assert tr2.micro_batch == 0 and tr2.state_dict()["accumulate"] == {"k": 3, "position": 0}
    tr2.close()
    assert _trainer().state_dict()["accumulate"] == {"k": 1, "position": 0}


def test_an_open_window_travels_by_parameter_name():
    """position > 0: the running sum is stored per parameter under the model's names and lands in the new trainer's accumulator"""
    tr = _trainer(accumulate_grad_batches=3)
    tr.micro_batch = 2
    tr.flat_acc.copy_(torch.arange(tr.total, dtype=torch.float32))
    sd = copy.deepcopy(tr.state_dict())
    assert sd["accumulate"]["position"] == 2 and set(sd["accumulate"]["sum"]) == {"weight", "bias"}
    assert sd["accumulate"]["sum"]["weight"].shape == (8, 8)
    want = tr.flat_acc.clone()
    tr.close()
    tr2 = _trainer(accumulate_grad_batches=3)
    tr2.load_state_dict(sd)
    assert tr2.micro_batch == 2 and torch.equal(tr2.flat_acc, want)
    del sd["accumulate"]["sum"]["bias"]
    with pytest.raises(KeyError, match="bias"):
        tr2.load_state_dict(sd)
    tr2.close()


def test_load_refuses_another_window_length_and_takes_older_states():
    tr = _trainer(accumulate_grad_batches=3)
    sd = copy.deepcopy(tr.state_dict())
    tr.close()
    for k in (1, 2):
        other = _trainer(accumulate_grad_batches=k)
        with pytest.raises(ValueError, match="accumulate_grad_batches=3"):
            other.load_state_dict(sd)
        other.close()
    old = {key: v for key, v in sd.items() if key != "accumulate"}     # a state written before there were windows
    tr3 = _trainer(accumulate_grad_batches=3)
    tr3.micro_batch = 1
    tr3.load_state_dict(old)
    assert tr3.micro_batch == 0
    tr3.close()
