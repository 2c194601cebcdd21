"""qt_attention_fp8_d32 / qt_value_codes_t_d32 without a GPU: declared, bound and built; the route rule against its profile; declined shapes."""
import os
import re

import pytest

from quantized_training import _native, attention_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,like", [("qt_attention_fp8_d32", "qt_attention_fp8"), ("qt_value_codes_t_d32", None)])
def test_symbols_are_declared_bound_and_built(name, like):
    with open(os.path.join(ROOT, "include", "qt_hip.h")) as f:
        decl = re.search(r"int %s\(([^;]*)\);" % name, f.read())
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]) and (like is None or _native.SIGNATURES[name] == _native.SIGNATURES[like])
    assert hasattr(_native.lib(), name) and _native.lib().qt_abi_version() == 3


def test_the_rule_agrees_with_the_committed_table():
    """A class (four rows: padding / no mask, eager / replayed) is taken exactly when the kernel beats the chain by more than its spread in all."""
    rows = {}
    with open(os.path.join(ROOT, "profiles", "attention_fp8_d32.txt")) as f:
        for line in f:
            m = re.match(r"B (\d+) H (\d+) S (\d+) D 32 \S+ +(eager|graph) +chain +([\d.]+) \(([\d.]+)-([\d.]+)\) us +kernel +([\d.]+) ", line)
            if m:
                B, H, S = map(int, m.group(1, 2, 3))
                chain, lo, hi, kernel = map(float, m.group(5, 6, 7, 8))
                rows.setdefault((B, H, S, S), []).append(chain - kernel > hi - lo)
    assert set(rows) == {(16, 4, 384, 384), (32, 4, 128, 128), (16, 4, 512, 512)} and all(len(v) == 4 for v in rows.values())
    for key, wins in rows.items():
        assert attention_route._fp8_d32_route_takes(*key) == all(wins), key
    assert set(k for k, v in attention_route._FP8_D32_TABLE.items() if v) <= set(rows) and not attention_route._fp8_d32_route_takes(3, 4, 256, 256)


def test_the_route_declines_what_the_kernel_does_not_take(monkeypatch):
    monkeypatch.setenv("QT_FUSED_ATTENTION", "1")
    core = attention_route._fp8_core_for
    assert [core(2, 4, C, C, 32) for C in (128, 512, 640, 64, 192)] == ["qt_attention_fp8_d32"] * 2 + [None] * 3 and core(2, 4, 128, 128, 64) == "qt_attention_fp8"
    monkeypatch.delenv("QT_FUSED_ATTENTION")
    assert core(2, 4, 128, 128, 32) is None and (core(32, 4, 128, 128, 32) is not None) == attention_route._fp8_d32_route_takes(32, 4, 128, 128)
