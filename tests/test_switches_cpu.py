"""The registry of environment switches (hulc2_amd/switches.py): the one reader of HULC_* variables in the Python layer, one truth rule,
unknown names refused, a scope that restores, a complete graph key — and the names bench.py, the tests and INTEGRATION.md use are its names."""
import os
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from hulc2_amd import switches  # noqa: E402

NAMES = [s.name for s in switches.TABLE]
BOOLS = [s for s in switches.TABLE if s.kind is bool]
VALUES = [s for s in switches.TABLE if s.kind is not bool]
IN_GRAPH = [s.name for s in switches.TABLE if s.in_graph]
NOT_IN_GRAPH = [s.name for s in switches.TABLE if not s.in_graph]


@pytest.fixture(autouse=True)
def no_switch_set(monkeypatch):
    for n in NAMES:
        monkeypatch.delenv(n, raising=False)


def test_the_table_is_well_formed():
    assert len(set(NAMES)) == len(NAMES) and len(switches._BY_KEY) == len(NAMES)      # (no short name stands for two switches)
    for s in switches.TABLE:
        assert re.fullmatch(r"HULC2?_[A-Z0-9_]+", s.name) and s.kind in (bool, str, int) and type(s.default) is s.kind, s
        assert s.read in ("call", "construction") and type(s.in_graph) is bool and s.doc, s


def test_switches_is_the_only_reader_of_the_environment():
    """the Python twin of test_host_cpu.py's csrc check: outside switches.py, lib.py (HULC_LIB) and build.py (HIPCC, HULC_BUILD_FLAGS) no file
    of the package holds a quoted variable name, nor a line that reads the environment and speaks of HULC"""
    allowed = {"switches.py", "lib.py", "build.py"}
    files = sorted((ROOT / "hulc2_amd").rglob("*.py"))
    assert len(files) > 30 and allowed <= {f.name for f in files}
    bad = []
    for f in files:
        if f.parent == ROOT / "hulc2_amd" and f.name in allowed:
            continue
        for i, line in enumerate(f.read_text().splitlines(), 1):
            if re.search(r"""["']HULC2?_[A-Z0-9_]+["']""", line) or (re.search(r"environ|getenv", line) and "HULC" in line):
                bad.append(f"{f.relative_to(ROOT)}:{i}: {line.strip()}")
    assert not bad, "\n".join(bad)


def test_every_read_in_the_package_names_a_switch_of_its_kind():
    """a path that runs on several ranks only, say, must not be where a misspelt or mis-kinded read is first met"""
    reads = []
    for f in sorted((ROOT / "hulc2_amd").rglob("*.py")):
        reads += re.findall(r"""switches\.(on|value|entry)\(\s*["']([^"']*)["']""", f.read_text())
    assert len(reads) >= len(NAMES) and {"on", "value", "entry"} == {how for how, _ in reads}
    tables = {"on": switches._BOOLS, "value": switches._VALUES, "entry": switches._BY_KEY}
    bad = [(how, key) for how, key in reads if key not in tables[how]]
    assert not bad, bad
    assert {key for _, key in reads} == set(switches._BY_KEY), "a registered switch that nothing reads, or the reverse"


@pytest.mark.parametrize("s", BOOLS, ids=lambda s: s.name)
def test_one_truth_rule_for_every_bool(s, monkeypatch):
    short = s.name.split("_", 1)[1]
    assert switches.on(short) is s.default
    for raw, want in (("", s.default), ("0", False), ("1", True)):
        monkeypatch.setenv(s.name, raw)
        assert switches.on(short) is want, (raw, want)
    with pytest.raises(KeyError):
        switches.value(short)                       # (a bool is read through on() alone)


@pytest.mark.parametrize("s", VALUES, ids=lambda s: s.name)
def test_values_are_the_default_or_what_was_set(s, monkeypatch):
    short = s.name.split("_", 1)[1]
    assert switches.value(short) == s.default and type(switches.value(short)) is s.kind
    want = 12 if s.kind is int else "a,b /c"
    monkeypatch.setenv(s.name, str(want))
    assert switches.value(short) == want and type(switches.value(short)) is s.kind
    with pytest.raises(KeyError):
        switches.on(short)                          # (the truthiness of a string or a number is no switch)


def test_unknown_names_are_refused():
    wrong = "HULC_NO_RNN_WAVEFRONTS"
    for name in (wrong, wrong.split("_", 1)[1], "HULC_NO_RNN_WAVEFRONT", "HULC_FP32_SITES"):      # (readers take the name without its prefix)
        with pytest.raises(KeyError):
            switches.on(name)
        with pytest.raises(KeyError):
            switches.value(name)
    with pytest.raises(KeyError):
        with switches.scope(NO_RNN_WAVEFRONT="1"):              # (scope takes the environment's own name)
            pass
    with pytest.raises(KeyError):
        with switches.scope(HULC_FORK="0", **{wrong: "1"}):
            pass
    assert "HULC_FORK" not in os.environ and wrong not in os.environ            # (refused before anything was set)


def test_scope_restores_the_environment(monkeypatch):
    monkeypatch.setenv("HULC_FORK", "0")
    monkeypatch.setenv("HULC_NO_STEP_NODE", "1")
    before = dict(os.environ)
    with switches.scope(HULC_FORK="1", HULC_NO_STEP_NODE=None, HULC_NO_MLP_CHAIN="1"):
        assert (os.environ["HULC_FORK"], os.environ["HULC_NO_MLP_CHAIN"]) == ("1", "1") and "HULC_NO_STEP_NODE" not in os.environ
        with switches.scope(HULC_FORK=None, HULC_NO_STEP_NODE="1", HULC_NO_MLP_CHAIN=None):
            assert "HULC_FORK" not in os.environ and "HULC_NO_MLP_CHAIN" not in os.environ and os.environ["HULC_NO_STEP_NODE"] == "1"
            assert switches.on("FORK") and switches.on("NO_STEP_NODE") and not switches.on("NO_MLP_CHAIN")
        assert (os.environ["HULC_FORK"], os.environ["HULC_NO_MLP_CHAIN"]) == ("1", "1") and "HULC_NO_STEP_NODE" not in os.environ
    assert dict(os.environ) == before
    with pytest.raises(ZeroDivisionError):
        with switches.scope(HULC_FORK=None, HULC_FP32_SITES="head"):
            with switches.scope(HULC_FP32_SITES=None):
                1 / 0
    assert dict(os.environ) == before


def test_graph_key_follows_every_in_graph_switch_and_no_other():
    assert set(IN_GRAPH) >= {"HULC_FP32_SITES", "HULC_NO_RNN_WAVEFRONT", "HULC_NO_MLP_CHAIN", "HULC_NO_FUSED_TXL", "HULC_NO_TXL_BLOCK",
                             "HULC_ENC_STREAMS", "HULC_NO_MODALITY_BATCHING", "HULC_FORK", "HULC_TRUNK_GRID"}
    base = switches.graph_key()
    assert len(base) == len(IN_GRAPH)
    seen = {base}
    for n in IN_GRAPH:
        with switches.scope(**{n: "1"}):
            key = switches.graph_key()
        assert key not in seen, n                   # (differs from the unset key and from every other switch's)
        seen.add(key)
    for n in NOT_IN_GRAPH:
        with switches.scope(**{n: "1"}):
            assert switches.graph_key() == base, n
    assert switches.graph_key() == base


def test_names_that_bench_and_the_tests_set_are_registered():
    bench = {"HULC_FP32_SITES", "HULC_NO_STEP_NODE", "HULC_ENC_STREAMS", "HULC_FORK", "HULC_NO_RNN_WAVEFRONT", "HULC_NO_MLP_CHAIN",
             "HULC_WGRAD_FORK"}
    assert bench <= set(NAMES), bench - set(NAMES)
    text = (ROOT / "bench.py").read_text()
    assert all(n in text for n in bench)
    # not switches of the package: the tests' own error recorder, bench.py's process settings, the emulation study's modes
    foreign = re.compile(r"HULC_RECORD_ERRORS|HULC_BENCH_\w+|HULC_EMU_\w+")
    used = set()
    for f in sorted((ROOT / "tests").rglob("*.py")):
        src = f.read_text()
        used |= set(re.findall(r"""setenv\(\s*["'](HULC2?_[A-Z0-9_]+)["']""", src))
        for call in re.findall(r"switches\.scope\(([^)]*)\)", src):
            used |= set(re.findall(r"\b(HULC2?_[A-Z0-9_]+)\s*=", call))
    assert len(used) > 10, used
    unknown = {n for n in used if not foreign.fullmatch(n)} - set(NAMES)
    assert not unknown, unknown


def test_the_document_lists_the_registry():
    doc = (ROOT / "INTEGRATION.md").read_text()
    section = doc[doc.index("\n## 4. Switches"):]
    listed = re.findall(r"^\| `(HULC2?_[A-Z0-9_]+)` \|", section, flags=re.M)
    assert listed == NAMES
