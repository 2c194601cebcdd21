"""The QT_* switch registry (quantized_training/switches.py): every product switch parses every raw value as the expression it
replaced did, reads the environment at call time, is the only place of the package that reads it, and matches README's table.

The expected columns below were written from the parent commit's expressions (quoted per kind), not from the registry; the rows of
`_public()` go through functions the parent already had, and that part of the table (test_public_accessors_*) passes on it unchanged."""
import ast
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "quantized-training_amd", "quantized_training")
RAW = [None, "", "0", "1", "2", "auto", "junk"]                      # None: unset

# kind -> what the parent computed for RAW, in order
ON_UNLESS_0 = [True, True, False, True, True, True, True]           # os.environ.get(NAME, "1") != "0"
OFF_UNLESS_1 = [False, False, False, True, False, False, False]     # os.environ.get(NAME, "0") == "1"
TRI = ["auto", "auto", "0", "1", "auto", "auto", "auto"]            # v = os.environ.get(NAME, "auto"); v if v in ("0", "1") else "auto"
LEVEL = ["1", "1", "0", "1", "2", "1", "1"]                         # QT_FQ8_MLP: == "0" never, == "2" always, anything else by the table
AS_SET = [None, "", "0", "1", "2", "auto", "junk"]                  # os.environ.get(NAME)

ON_SWITCHES = ["QT_FP8_GEMM", "QT_LT_GEMM", "QT_SIBLING_GEMM", "QT_GATE_UP_GROUP", "QT_FUSED_SOFTMAX", "QT_FP8_ATTENTION", "QT_FP8_ATTENTION_KERNEL",
               "QT_ROPE_VALUE_LAUNCH", "QT_ROPE_WEIGHT_PASS", "QT_FUSED_MODEL_OPS", "QT_FUSED_PRODUCER_FQ", "QT_FUSED_PRODUCER_MAP", "QT_CODES_ONLY",
               "QT_PT2E_FUSE", "QT_PT2E_NATIVE", "QT_MX_GEMM", "QT_TRAIN_GEMM"]
OFF_SWITCHES = ["QT_FUSED_GEMM", "QT_LAZY_POISON"]
TRI_SWITCHES = ["QT_FQ8_GEMM", "QT_FQT_GEMM", "QT_FUSED_ATTENTION", "QT_CONV_GEMM"]
RAW_SWITCHES = ["QT_LT_ALGO", "QT_HIP_LIB"]


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _table(monkeypatch, name, read, expected, raws=RAW):
    for value, want in zip(raws, expected, strict=True):
        _set(monkeypatch, name, value)
        got = read()
        assert got == want and type(got) is type(want), (name, value, got, want)


def test_registry_lists_the_27_product_switches_once():
    from quantized_training import switches
    product = [n for n, row in switches.SWITCHES.items() if row[2] == "product"]
    assert sorted(product) == sorted(ON_SWITCHES + OFF_SWITCHES + TRI_SWITCHES + RAW_SWITCHES + ["QT_FQ8_MLP", "QT_TRAIN_DEBUG"]) and len(product) == 27
    assert {n for n, row in switches.SWITCHES.items() if row[2] == "native"} == {"QT_MX_WIDE", "QT_MX_WIDE_TM"}
    assert {n for n, row in switches.SWITCHES.items() if row[2] == "bench"} == {"QT_BENCH_DROPOUT", "QT_BENCH_NO_OBSERVE"}
    assert all(len(row) == 4 and row[3] for row in switches.SWITCHES.values())
    for read in (switches.on, switches.mode, switches.raw, lambda n: switches.mask(n, {})):
        with pytest.raises(KeyError):
            read("QT_NO_SUCH_SWITCH")


def test_every_product_switch_parses_every_raw_value_as_before(monkeypatch):
    from quantized_training import switches
    for name in ON_SWITCHES:
        _table(monkeypatch, name, lambda: switches.on(name), ON_UNLESS_0)
    for name in OFF_SWITCHES:
        _table(monkeypatch, name, lambda: switches.on(name), OFF_UNLESS_1)
    for name in TRI_SWITCHES:
        _table(monkeypatch, name, lambda: switches.mode(name), TRI)
        _table(monkeypatch, name, lambda: switches.on(name), ON_UNLESS_0)       # the raw `== "0"` / `!= "0"` sites (QT_FUSED_ATTENTION, fq8_gemm_enabled)
    _table(monkeypatch, "QT_FQ8_MLP", lambda: switches.mode("QT_FQ8_MLP"), LEVEL)
    _table(monkeypatch, "QT_FQ8_MLP", lambda: switches.on("QT_FQ8_MLP"), ON_UNLESS_0)
    for name in RAW_SWITCHES:
        _table(monkeypatch, name, lambda: switches.raw(name), AS_SET)
    # int(os.environ.get("QT_TRAIN_DEBUG", "0") or "0", 0), ValueError with the mask's names otherwise
    bits = {"chains": 1}
    _table(monkeypatch, "QT_TRAIN_DEBUG", lambda: switches.mask("QT_TRAIN_DEBUG", bits), [0, 0, 0, 1, 2, 16], [None, "", "0", "1", "2", "0x10"])
    for bad in ("auto", "junk", "abc"):
        monkeypatch.setenv("QT_TRAIN_DEBUG", bad)
        with pytest.raises(ValueError, match=re.escape(f"QT_TRAIN_DEBUG={bad!r}: an integer mask of {bits}")):
            switches.mask("QT_TRAIN_DEBUG", bits)


def _public():
    """(switch, function the parent already had, expected column)."""
    from quantized_training import conv_route, fused, mx_gemm, train_fusions
    return [("QT_FQ8_GEMM", fused.fq8_gemm_mode, TRI), ("QT_FQT_GEMM", fused.fqt_gemm_mode, TRI), ("QT_CONV_GEMM", conv_route.conv_gemm_mode, TRI),
            ("QT_FQ8_GEMM", fused.fq8_gemm_enabled, ON_UNLESS_0), ("QT_FUSED_GEMM", fused.fused_gemm_enabled, OFF_UNLESS_1),
            ("QT_FP8_GEMM", fused.fp8_gemm_enabled, ON_UNLESS_0), ("QT_MX_GEMM", mx_gemm._enabled, ON_UNLESS_0),
            ("QT_TRAIN_DEBUG", lambda: train_fusions._on("chains"), [True, True, True, False, True]),
            ("QT_TRAIN_DEBUG", lambda: train_fusions._on("fanin"), [True, True, True, True, True])]


def test_public_accessors_keep_their_results(monkeypatch):
    from quantized_training import train_fusions
    for name, read, expected in _public():
        _table(monkeypatch, name, read, expected, RAW[:len(expected)])
    monkeypatch.setenv("QT_TRAIN_DEBUG", "0x10")
    assert train_fusions._on("chains") and not train_fusions._on("fanin") and train_fusions.producers_enabled() and not train_fusions.fanin_enabled()
    for bad in ("auto", "junk", "abc"):
        monkeypatch.setenv("QT_TRAIN_DEBUG", bad)
        with pytest.raises(ValueError, match=re.escape(f"QT_TRAIN_DEBUG={bad!r}: an integer mask of {train_fusions.DEBUG_BITS}")):
            train_fusions.enabled()


def test_public_accessors_read_the_environment_at_call_time(monkeypatch):
    from quantized_training import fused, train_fusions
    monkeypatch.delenv("QT_FQ8_GEMM", raising=False)
    monkeypatch.delenv("QT_TRAIN_DEBUG", raising=False)
    assert fused.fq8_gemm_mode() == "auto" and fused.fq8_gemm_enabled() and train_fusions.enabled()
    monkeypatch.setenv("QT_FQ8_GEMM", "0")
    monkeypatch.setenv("QT_TRAIN_DEBUG", "1")
    assert fused.fq8_gemm_mode() == "0" and not fused.fq8_gemm_enabled() and not train_fusions.enabled()
    monkeypatch.setenv("QT_FQ8_GEMM", "1")
    monkeypatch.delenv("QT_TRAIN_DEBUG")
    assert fused.fq8_gemm_mode() == "1" and train_fusions.enabled()


def _package_sources():
    for folder, _, names in os.walk(PKG):
        for n in sorted(names):
            if n.endswith(".py"):
                path = os.path.join(folder, n)
                with open(path) as f:
                    yield os.path.relpath(path, PKG), ast.parse(f.read())


def test_only_switches_py_reads_the_environment_for_a_qt_name():
    """Outside switches.py: no call, subscript or comparison that touches os.environ / os.getenv and names a QT_ switch, and no
    `from os import environ / getenv`."""
    found = []
    for rel, tree in _package_sources():
        if rel == "switches.py":
            continue
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module == "os" and {a.name for a in node.names} & {"environ", "getenv"}:
                found.append((rel, node.lineno))
            if isinstance(node, (ast.Call, ast.Subscript, ast.Compare)):
                inner = list(ast.walk(node))
                reads = any(isinstance(n, ast.Attribute) and n.attr in ("environ", "getenv") for n in inner)
                if reads and any(isinstance(n, ast.Constant) and isinstance(n.value, str) and "QT_" in n.value for n in inner):
                    found.append((rel, node.lineno))
    assert not found, found


HOOK_DICTS = {"_forward_hooks", "_forward_pre_hooks", "_backward_hooks", "_backward_pre_hooks"}


def test_hook_dicts_are_named_in_three_places_only():
    """planner_checks.py, quantize.py (removes the hooks it registered), model_fusions._run_pre_hooks (executes them)."""
    found = []
    for rel, tree in _package_sources():
        if rel in ("planner_checks.py", "quantize.py"):
            continue
        allowed = set()
        if rel == "model_fusions.py":
            fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_run_pre_hooks")
            allowed = {id(n) for n in ast.walk(fn)}
        for n in ast.walk(tree):
            named = (isinstance(n, ast.Attribute) and n.attr in HOOK_DICTS) or (isinstance(n, ast.Constant) and n.value in HOOK_DICTS)
            if named and id(n) not in allowed:
                found.append((rel, n.lineno))
    assert not found, found
    gone = [("model_fusions.py", "_hooked"), ("model_fusions.py", "_only_pre_hooks"), ("fused.py", "_has_table_hooks"), ("fused.py", "_has_hooks"),
            ("train_fusions.py", "_hooked")]
    trees = dict(_package_sources())
    assert not [(f, name) for f, name in gone if any(isinstance(n, ast.FunctionDef) and n.name == name for n in trees[f].body)]


def test_readme_switch_table_names_the_registry():
    from quantized_training import switches
    with open(os.path.join(ROOT, "README.md")) as f:
        text = f.read()
    section = text.split("### Environment switches", 1)[1]
    rows = [line for line in section.splitlines() if line.startswith("|")]
    names = {n for line in rows for n in re.findall(r"QT_[A-Z0-9_]*[A-Z0-9]", line) if f"{n}_*" not in line}      # (`QT_TRAIN_*`: a family of the past)
    assert names == set(switches.SWITCHES), (sorted(names - set(switches.SWITCHES)), sorted(set(switches.SWITCHES) - names))
    product = sum(1 for row in switches.SWITCHES.values() if row[2] == "product")
    assert f"the package reads {product} switches" in text and "quantized_training/switches.py" in section
