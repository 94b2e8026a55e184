"""Every HULC_* / HULC2_* environment switch of the Python layer: one table, one truth rule, one reader.

The environment is the only store.  Every accessor reads it at the moment of the call: nothing is cached and there is no second override
layer, so a program that writes os.environ between two steps (bench.py does, between legs) is honoured by the next read.  No other module
of the package reads a HULC_* variable, except lib.py (HULC_LIB) and build.py (HIPCC, HULC_BUILD_FLAGS): those choose WHICH library is
loaded, not what it does.  The C side reads no environment at all (include/hulc2_amd.h).

One spelling per use: the readers on(), value() and entry() take the name without its prefix (`on("NO_MLP_CHAIN")`: no other module of
the package holds a variable's name), scope() and graph_key() speak of the environment and take / follow the full names.  A name that is
not in the table is a KeyError, never a silent default — and so is on() of a switch that is no `bool`, or value() of one that is.

Truth rule of every `bool` switch: unset or empty = the default, "0" = off, anything else = on.  Two differences to the reads this module
replaced, neither reachable by a value that anything in the project sets:
  - a HULC_NO_* flag set to "0" is off (the bare `os.environ.get(X)` read took "0" for on);
  - HULC_TRUNK_GRID is on for every value that is not off, not for "1" alone.
An `int` switch goes through int().  HULC_RNN_DBG used to take everything but plain digits for 0: a value that is no number is now a
ValueError at the launch that reads it, and " 4" or "-4" count as int() reads them (bit 4 set).  An empty HULC_ALLREDUCE means auto (it was
a ValueError).

`read` is the moment the value takes effect: at every `call` of the function that asks, or at the `construction` of the object named in
the description (set it before that object is made).  `in_graph`: the value decides which launches a training step issues or what their
descriptors hold; graph_key() is part of the step node's capture signature (stepnode.StepNode._signature), so flipping one of them on a
live model leads to a new capture, not to the replay of a graph recorded under the other setting.
"""
import os
from contextlib import contextmanager
from typing import NamedTuple, Union


class Switch(NamedTuple):
    name: str                           # the environment variable
    kind: type                          # bool | str | int
    default: Union[bool, str, int]
    read: str                           # "call" | "construction"
    in_graph: bool
    doc: str


TABLE = (
    # --- what a training step launches (all in the step node's capture signature) ---
    Switch("HULC_FP32_SITES", str, "head,goal,encfc,txl", "call", True, "parts of a bf16 step whose forward runs in exact fp32, comma separated (kernels.fp32_sites)"),
    Switch("HULC_FP32_SITES_BWD", bool, False, "call", True, "the selected sites run their backward in exact fp32 too"),
    Switch("HULC_FORK", bool, True, "call", True, "prior and posterior branch of a step on two streams; 0: one after the other"),
    Switch("HULC_WGRAD_FORK", bool, False, "call", True, "recurrent weight gradients as a third branch beside the data-gradient chain (native trainer only; not taken with policy_rnn_dropout_p > 0)"),
    Switch("HULC_NO_MLP_CHAIN", bool, False, "call", True, "per-layer GEMMs in place of the chained MLP kernel"),
    Switch("HULC_NO_MLP2_ROWS", bool, False, "call", True, "per-layer GEMMs in place of the camera encoders' fused fc1-ReLU-fc2 head"),
    Switch("HULC_TXL_NO_SHARE", bool, False, "call", True, "the whole-trunk transformer launch keeps one workgroup per sequence"),
    Switch("HULC_RNN_DBG", int, 0, "call", True, "bit 4: the recurrent wavefront launch ends as if a barrier had timed out (tests of the fault path)"),
    Switch("HULC_CONV1_PER_INPUT", bool, False, "call", True, "one conv1 launch per camera in place of the paired launch"),
    Switch("HULC_NO_FUSED_TXL", bool, False, "call", True, "transformer layers as the unfused kernel chain, not the fused layer launch"),
    Switch("HULC_NO_FUSED_FFN", bool, False, "call", True, "the feed-forward network of a transformer layer as separate GEMMs (also turns the fused layer launch off)"),
    Switch("HULC_NO_TXL_BLOCK", bool, False, "call", True, "one launch per transformer layer in place of the whole-trunk launch"),
    Switch("HULC_NO_RNN_WAVEFRONT", bool, False, "call", True, "per-step GEMMs in place of the persistent recurrent wavefront kernel"),
    Switch("HULC_RNN_WGRAD_TMIRROR", bool, False, "call", True, "the recurrent sweep keeps transposed (feature-major) mirrors for the weight-gradient GEMMs (not taken with policy_rnn_dropout_p > 0)"),
    Switch("HULC_ENC_STREAMS", bool, True, "call", True, "the two camera encoders on two streams; 0: one stream"),
    Switch("HULC_NO_MODALITY_BATCHING", bool, False, "call", True, "one pass per modality in place of one batched pass over vision and language windows"),
    Switch("HULC_FULL_ZERO_GRAD", bool, False, "call", True, "zero the whole gradient arena every step, not only the ranges no kernel overwrites"),
    Switch("HULC_NO_FRAME_SLOTS", bool, False, "call", True, "the step node copies frames into its static inputs in place of the in-place frame slots (read at capture)"),
    Switch("HULC_TRUNK_GRID", bool, False, "call", True, "R3M trunk (real-world config): the stride-1 3 x 3 convolutions on the padded grid (bf16)"),
    # --- which loop runs a step, and everything outside the step ---
    Switch("HULC_NO_STEP_GRAPH", bool, False, "construction", False, "StepNode: the eager node, no hipGraph capture"),
    Switch("HULC_NO_STEP_NODE", bool, False, "call", False, "no step node: the weight keeper holds weight copies only (read when a model first makes its keeper)"),
    Switch("HULC_NO_AUTO_SHADOWS", bool, False, "call", False, "no weight keeper: lazy per-parameter bf16 copies"),
    Switch("HULC_TORCH_ADAM", bool, False, "call", False, "configure_optimizers hands out torch's optimizer classes, not the fused arena drop-ins"),
    Switch("HULC_ALLREDUCE", str, "", "construction", False, "GradComm: gradient all-reduce algorithm, auto | ring | direct; empty: auto, and a resumed run keeps its checkpoint's"),
    Switch("HULC_GRAD_PAYLOAD", str, "", "construction", False, "GradComm: gradient payload on the wire, fp32 | bf16; empty: by world size"),
    Switch("HULC_FAULT_CHECK_EVERY", int, 64, "construction", False, "ArenaTrainer: steps between two reads of the device fault word"),
    Switch("HULC_CAPTURE_MODE", str, "thread_local", "call", False, "ArenaTrainer.capture: capture_error_mode of a multi-rank graph capture"),
    Switch("HULC_NO_SPLIT_GRAPH", bool, False, "call", False, "ArenaTrainer.capture: one graph per step on several ranks, not one before and one after the all-reduce"),
    Switch("HULC_AFF_FROZEN_STEM", bool, False, "call", False, "affordance detector (trunk_mode reference, training): the stem runs with the frozen trunk, without its own backward"),
    Switch("HULC2_R3M_WEIGHTS", str, "", "call", False, "path of an r3m model.pt for VisionR3M"),
    Switch("HULC2_SBERT_DIR", str, "", "call", False, "directory with the sentence encoder's files"),
)

_BY_NAME = {s.name: s for s in TABLE}                              # scope(): the environment's own names
_BY_KEY = {s.name.split("_", 1)[1]: s for s in TABLE}              # the readers: the name without its prefix
_BOOLS = {k: s for k, s in _BY_KEY.items() if s.kind is bool}      # on() knows only these, value() only the others
_VALUES = {k: s for k, s in _BY_KEY.items() if s.kind is not bool}
_IN_GRAPH = tuple(s.name for s in TABLE if s.in_graph)


def entry(key: str) -> Switch:
    return _BY_KEY[key]


def on(key: str) -> bool:
    """a `bool` switch, by the truth rule above"""
    s = _BOOLS[key]
    v = os.environ.get(s.name)
    return s.default if not v else v != "0"


def value(key: str):
    """a `str` switch as it stands, or an `int` switch through int(); the default when unset (`int`: or empty)"""
    s = _VALUES[key]
    v = os.environ.get(s.name)
    if s.kind is int:
        return int(v) if v else s.default
    return s.default if v is None else v


def graph_key() -> tuple:
    """the raw values of every in_graph switch, in table order"""
    get = os.environ.get
    return tuple(get(n) for n in _IN_GRAPH)


@contextmanager
def scope(**env):
    """`with scope(HULC_FORK="0", HULC_NO_STEP_NODE=None):` sets (None: unsets) the ENVIRONMENT VARIABLES and puts them back on exit"""
    old = {_BY_NAME[k].name: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            _set(k, v)
        yield
    finally:
        for k, v in old.items():
            _set(k, v)


def _set(name, v):
    if v is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = v
