"""KL annealing, host side (reference: hulc2/utils/kl_callbacks.py:5-60, conf/callbacks/kl_schedule/*.yaml): the three rules of
`hulc2_amd.kl_schedule` against values recorded from the reference's callbacks (tests/golden/kl_schedule.json, written by
tools/gen_kl_schedule_golden.py), the four device-beta entry points of the C ABI, `Hulc2.set_kl_beta` on a CPU model, and the native loop's
`set_kl_schedule` / `begin_epoch`."""
import ctypes
import json
import struct
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from hulc2_amd import kl_schedule  # noqa: E402

FIXTURE = json.loads((ROOT / "tests" / "golden" / "kl_schedule.json").read_text())
SETS = [(s["start_epoch"], s["end_epoch"], float.fromhex(s["max_kl_beta"])) for s in FIXTURE["sets"]]


def _recorded(i, kind):
    return [float.fromhex(h) for h in FIXTURE["sets"][i][kind]]


def _f32_ulps(a: float, b: float) -> int:
    """distance of two non-negative floats in float32 steps, after rounding each to float32"""
    ia, ib = (struct.unpack("<i", struct.pack("<f", x))[0] for x in (a, b))
    return abs(ia - ib)


def test_fixture_holds_the_three_parameter_sets_and_61_epochs():
    assert SETS == [(10, 50, 0.01), (0, 5, 1.0), (3, 4, 0.5)]
    assert FIXTURE["epochs"] == 61 and all(len(s[k]) == 61 for s in FIXTURE["sets"] for k in ("linear", "sigmoid"))
    assert FIXTURE["constant"]["set_kl_beta_calls"] == 0
    ref = _recorded(0, "sigmoid")            # the shipped yamls with loss.kl_beta = 0.01
    assert _recorded(0, "linear")[11] == 0.00025
    assert (ref[10], ref[50], ref[51]) == (2.4726230185478927e-05, 0.009975274205207826, 0.01)


@pytest.mark.parametrize("i", range(3))
def test_linear_equals_the_reference_exactly(i):
    start, end, top = SETS[i]
    fn = kl_schedule.linear(start, end, top)
    got, want = [fn(e) for e in range(61)], _recorded(i, "linear")
    assert got == want, [(e, a, b) for e, (a, b) in enumerate(zip(got, want)) if a != b][:5]
    assert all(v == 0.0 for v in got[:start]) and got[end] == top and all(v == top for v in got[end:])


@pytest.mark.parametrize("i", range(3))
def test_sigmoid_equals_the_reference_within_two_float32_ulps(i):
    """the reference evaluates torch.sigmoid in float32, whose last bit may differ between CPU vector instruction sets: 2 float32 ulps of
    the recorded sigmoid value (the product with max_kl_beta is formed in doubles on both sides); exact where the fixture holds 0.0 or max"""
    start, end, top = SETS[i]
    fn = kl_schedule.sigmoid(start, end, top)
    got, want = [fn(e) for e in range(61)], _recorded(i, "sigmoid")
    for e, (a, b) in enumerate(zip(got, want)):
        if b == 0.0 or b == top:
            assert a == b, (e, a, b)
        else:
            assert _f32_ulps(a / top, b / top) <= 2, (e, a, b)
    assert all(v == 0.0 for v in got[:start]) and all(v == top for v in got[end + 1:])
    assert 0.0 < got[start] < got[end] < top                   # sigmoid(-6) max at start, sigmoid(6) max at end: the jump to max comes after it
    assert _f32_ulps(got[end] / top, torch.sigmoid(torch.tensor([6.0])).item()) <= 2


def test_constant_never_sets_the_weight():
    fn = kl_schedule.constant()
    assert all(fn(e) is None for e in range(61))
    with pytest.raises(ValueError):
        kl_schedule.linear(5, 5, 0.01)
    with pytest.raises(ValueError):
        kl_schedule.sigmoid(5, 4, 0.01)


def test_sched_entry_points_are_declared_and_exported():
    from hulc2_amd import build, lib

    build.build(verbose=False)
    so = lib.load()
    i, f, u, p = ctypes.c_int, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_void_p
    # the scalar twins, unchanged
    assert list(so.hulc_cat_kl_fwd.argtypes) == [p, p, i, i, i, f, i, p, p, p]
    assert list(so.hulc_cat_kl_bwd.argtypes) == [p, p, p, i, i, i, f, f, p, i, p, p, p]
    assert list(so.hulc_gauss_plan_fwd.argtypes) == [p, p, p, u, p, i, i, f, f, i, p, p, p, p, p]
    assert list(so.hulc_gauss_plan_bwd.argtypes) == [p, p, p, u, p, i, i, f, f, f, i, p, p, p, p, p]
    # the device-beta entries: the twin's arguments, then beta_dev in front of the stream
    assert list(so.hulc_cat_kl_fwd_sched.argtypes) == [p, p, i, i, i, f, i, p, p, p, p]
    assert list(so.hulc_cat_kl_bwd_sched.argtypes) == [p, p, p, i, i, i, f, f, p, i, p, p, p, p]
    assert list(so.hulc_gauss_plan_fwd_sched.argtypes) == [p, p, p, u, p, i, i, f, f, i, p, p, p, p, p, p]
    assert list(so.hulc_gauss_plan_bwd_sched.argtypes) == [p, p, p, u, p, i, i, f, f, f, i, p, p, p, p, p, p]
    for name in ("hulc_cat_kl_fwd_sched", "hulc_cat_kl_bwd_sched", "hulc_gauss_plan_fwd_sched", "hulc_gauss_plan_bwd_sched"):
        assert getattr(so, name).restype is ctypes.c_int
    assert so.hulc_abi_version() == 7


def test_sched_launchers_refuse_a_missing_or_misaligned_beta_dev_on_the_host():
    """the guards sit in front of every launch: they answer without a GPU (-1 null, -4 misaligned; the message names the entry point)"""
    from hulc2_amd import build, lib

    build.build(verbose=False)
    so = lib.load()
    so.hulc_last_error.restype = ctypes.c_char_p
    buf = ctypes.create_string_buffer(64)                      # host memory standing in for operands: nothing is launched
    a = ctypes.addressof(buf)
    assert so.hulc_cat_kl_fwd_sched(a, a, 2, 3, 32, 0.5, 1, a, a, None, None) == -1
    assert so.hulc_last_error() == b"hulc_cat_kl_fwd_sched: null beta_dev"
    assert so.hulc_cat_kl_fwd_sched(a, a, 2, 3, 32, 0.5, 1, a, a, a + 2, None) == -4
    assert so.hulc_last_error() == b"hulc_cat_kl_fwd_sched: beta_dev must be 4-byte aligned"
    assert so.hulc_cat_kl_bwd_sched(a, a, a, 2, 3, 32, 0.5, 0.8, a, 1, a, a, None, None) == -1
    assert so.hulc_last_error() == b"hulc_cat_kl_bwd_sched: null beta_dev"
    assert so.hulc_cat_kl_bwd_sched(a, a, a, 2, 3, 32, 0.5, 0.8, a, 1, a, a, a + 1, None) == -4
    assert so.hulc_gauss_plan_fwd_sched(a, a, a, 0, None, 2, 3, 1e-4, 0.5, 1, a, None, a, a, None, None) == -1
    assert so.hulc_last_error() == b"hulc_gauss_plan_fwd_sched: null beta_dev"
    assert so.hulc_gauss_plan_fwd_sched(a, a, a, 0, None, 2, 3, 1e-4, 0.5, 1, a, None, a, a, a + 2, None) == -4
    assert so.hulc_gauss_plan_bwd_sched(a, a, a, 0, None, 2, 3, 1e-4, 0.5, 0.8, 1, a, a, a, a, None, None) == -1
    assert so.hulc_last_error() == b"hulc_gauss_plan_bwd_sched: null beta_dev"
    assert so.hulc_gauss_plan_bwd_sched(a, a, a, 0, None, 2, 3, 1e-4, 0.5, 0.8, 1, a, a, a, a, a + 3, None) == -4
    assert so.hulc_last_error() == b"hulc_gauss_plan_bwd_sched: beta_dev must be 4-byte aligned"


def test_set_kl_beta_on_a_cpu_model_stores_the_float_only():
    """no device tensor, no new state_dict key; compute_kl_loss hands the FLOAT to the distribution.  The KL kernels themselves have no CPU
    path (a CPU tensor raises), so the distribution's kernel entry is replaced by a stand-in that records the weight it is handed; the VALUE
    of compute_kl_loss is compared with oracle.kl_loss where the kernels run, in tests/test_kl_beta_gpu.py."""
    from hulc2_amd.compat import instantiate
    from hulc2_amd.config import default_model_config
    from hulc2_amd.lib import HulcKernelError
    from hulc2_amd.utils.distributions import DiscState
    from oracle import hulc2_oracle as O

    m = instantiate(default_model_config())
    keys = set(m.state_dict())
    assert m.kl_beta == 0.01 and m._kl_beta_dev is None and not m.kl_beta_on_device
    m.set_kl_beta(0.00025)
    assert m.kl_beta == 0.00025 and type(m.kl_beta) is float
    assert m._kl_beta_dev is None and not m.kl_beta_on_device and m._kl_beta_arg() == 0.00025
    assert set(m.state_dict()) == keys and not any("kl_beta" in n for n, _ in m.named_buffers())
    g = torch.Generator().manual_seed(5)
    pp, pr = DiscState(torch.randn(3, 1024, generator=g)), DiscState(torch.randn(3, 1024, generator=g))
    with pytest.raises(HulcKernelError):                       # no CPU fallback, with or without a set weight
        m.compute_kl_loss(pp, pr)
    seen = []

    def by_oracle(pp_state, pr_state, kl_beta, mix):
        seen.append(kl_beta)
        return O.kl_loss(pp_state.logit, pr_state.logit, kl_beta, mix)

    m.dist.kl_balanced = by_oracle
    m.compute_kl_loss(pp, pr)
    assert seen == [0.00025] and type(seen[0]) is float      # the weight that reaches the distribution is the set float, by value


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 3)
        self.kl_beta = 0.01
        self.calls = []

    def set_kl_beta(self, kl_beta):
        self.calls.append(kl_beta)
        self.kl_beta = kl_beta


def test_trainer_schedule_calls_set_kl_beta_with_the_scheduled_values():
    from hulc2_amd.trainer import ArenaTrainer

    m = _StubModel()
    tr = ArenaTrainer(m)
    keys = set(tr.state_dict())
    tr.begin_epoch(0)                                          # no schedule attached: nothing happens
    assert m.calls == []
    tr.set_kl_schedule(kl_schedule.constant())
    for e in range(3):
        tr.begin_epoch(e)
    assert m.calls == [] and m.kl_beta == 0.01                 # the constant rule never sets the weight
    fn = kl_schedule.linear(10, 50, 0.01)
    tr.set_kl_schedule(fn)
    for e in (0, 9, 10, 11, 50, 51):
        tr.begin_epoch(e)
    assert m.calls == [fn(e) for e in (0, 9, 10, 11, 50, 51)] == [0.0, 0.0, 0.0, 0.00025, 0.01, 0.01]
    tr.set_kl_beta(0.5)
    assert m.calls[-1] == 0.5 and m.kl_beta == 0.5
    assert set(tr.state_dict()) == keys
