"""qt_attention_fp8_ragged / qt_value_codes_t_ragged without a GPU: exported and bound; the route over a grid of shapes; the rule against its profile."""
import os
import re

import pytest

from quantized_training import _native, attention_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = {(16, 12, 197, 197, 64), (32, 12, 77, 77, 64), (32, 12, 136, 136, 64), (32, 12, 200, 200, 64), (16, 12, 300, 300, 64), (16, 16, 376, 376, 64),
           (4, 32, 200, 200, 128)}


@pytest.mark.parametrize("name,like", [("qt_attention_fp8_ragged", "qt_attention_fp8"), ("qt_value_codes_t_ragged", "qt_value_codes_t")])
def test_symbols_are_exported_and_prototyped(name, like):
    assert _native.SIGNATURES[name] == _native.SIGNATURES[like]
    assert hasattr(_native.lib(), name) and _native.lib().qt_abi_version() == 3


def test_the_route_over_a_grid(monkeypatch):
    """Ragged C <= 512 at head_dim 64 / 128: the new entry, only when forced or listed; multiples of 128 and C > 512 as before."""
    core = attention_route._fp8_core_for
    ragged, unchanged = (1, 77, 197, 200, 511), {128: "qt_attention_fp8", 384: "qt_attention_fp8", 1024: "qt_attention_fp8", 513: None, 1100: None}
    monkeypatch.setenv("QT_FUSED_ATTENTION", "1")
    for D in (64, 128):
        assert [core(2, 4, C, C, D) for C in ragged] == ["qt_attention_fp8_ragged"] * len(ragged)
        assert {C: core(2, 4, C, C, D) for C in unchanged} == unchanged
    assert core(2, 4, 197, 197, 32) is None and core(2, 4, 197, 197, 96) is None and core(65536, 1, 197, 197, 64) is None
    assert core(2, 4, 2048, 2048, 128) == "qt_attention_fp8_long" and core(2, 4, 128, 128, 32) == "qt_attention_fp8_d32"
    monkeypatch.delenv("QT_FUSED_ATTENTION")
    for D in (64, 128):
        assert [core(2, 4, C, C, D) for C in ragged] == [None] * len(ragged)              # (2, 4, ...) is no measured class
        assert {C: core(2, 4, C, C, D) for C in unchanged} == unchanged
    for key in CLASSES:
        assert (core(*key) == "qt_attention_fp8_ragged") == attention_route._fp8_ragged_route_takes(*key), key


def test_the_rule_agrees_with_the_committed_table():
    """A class (four rows: padding / no mask, eager / replayed) is taken exactly when the kernel beats the parent's route by more than its spread in all."""
    rows = {}
    with open(os.path.join(ROOT, "profiles", "attention_fp8_ragged.txt")) as f:
        for line in f:
            m = re.match(r"B (\d+) H (\d+) S (\d+) D (\d+) \S+ +(eager|graph) +parent +([\d.]+) \(([\d.]+)-([\d.]+)\) us +kernel +([\d.]+) ", line)
            if m:
                B, H, S, D = map(int, m.group(1, 2, 3, 4))
                parent, lo, hi, kernel = map(float, m.group(6, 7, 8, 9))
                rows.setdefault((B, H, S, S, D), []).append(parent - kernel > hi - lo)
    assert all(len(v) == 4 for v in rows.values())
    for key, wins in rows.items():
        assert attention_route._fp8_ragged_route_takes(*key) == all(wins), key
    assert set(k for k, v in attention_route._FP8_RAGGED_TABLE.items() if v) <= set(rows) & CLASSES and not attention_route._fp8_ragged_route_takes(3, 4, 197, 197, 64)
