"""qt_attention_fp8_gqa without a GPU: exported, declared and bound; the G = 1 routes as they were; the grouped rule against its table and its
profile; the grouped route's shape check on the host."""
import os
import re

import pytest

from quantized_training import _native, attention_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_exported_declared_and_prototyped():
    sig, like = _native.SIGNATURES["qt_attention_fp8_gqa"], _native.SIGNATURES["qt_attention_fp8_long"]
    assert sig[0] == like[0] and sig[1] == like[1][:19] + [like[1][18]] + like[1][19:]          # qt_attention_fp8_long's list plus Hkv behind H
    assert hasattr(_native.lib(), "qt_attention_fp8_gqa") and _native.lib().qt_abi_version() == 3
    with open(os.path.join(ROOT, "include", "qt_hip.h")) as f:
        assert re.search(r"int qt_attention_fp8_gqa\([^;]*long B, int H, int Hkv, int Sq, int Sk, int head_dim, float scaling, void \*stream\);", f.read())


def test_the_ungrouped_routes_are_as_they_were(monkeypatch):
    """_fp8_core_for on every shape of the three committed G = 1 tables, and at the borders between its cores."""
    monkeypatch.delenv("QT_FUSED_ATTENTION", raising=False)
    core = attention_route._fp8_core_for
    for table, entry, shape in ((attention_route._FP8_LONG_TABLE, "qt_attention_fp8_long", lambda k: k),
                                (attention_route._FP8_D32_TABLE, "qt_attention_fp8_d32", lambda k: (*k, 32)),
                                (attention_route._FP8_RAGGED_TABLE, "qt_attention_fp8_ragged", lambda k: k)):
        assert table and all(core(*shape(k)) == entry for k in table), entry
    assert [core(1, 32, C, C, 128) for C in (128, 1024, 1152, 197)] == ["qt_attention_fp8", "qt_attention_fp8", None, None]
    monkeypatch.setenv("QT_FUSED_ATTENTION", "1")
    assert [core(1, 32, C, C, 128) for C in (1024, 1152, 197)] == ["qt_attention_fp8", "qt_attention_fp8_long", "qt_attention_fp8_ragged"]


def test_the_rule_agrees_with_its_table_and_its_profile(monkeypatch):
    """Every row of _FP8_GQA_TABLE is what the rule says, and a class (four rows: causal / no mask, eager / replayed) is listed exactly when
    the kernel route beats the parent's by more than the parent's spread in all four."""
    monkeypatch.delenv("QT_FUSED_ATTENTION", raising=False)
    for key, taken in attention_route._FP8_GQA_TABLE.items():
        assert attention_route._fp8_gqa_route_takes(*key) == taken
        assert (attention_route._fp8_gqa_core_for(*key) == "qt_attention_fp8_gqa") == taken
    rows = {}
    with open(os.path.join(ROOT, "profiles", "attention_fp8_gqa.txt")) as f:
        for line in f:
            m = re.match(r"B (\d+) H (\d+) Hkv (\d+) S (\d+) D (\d+) \S+ +(eager|graph) +parent +([\d.]+) \(([\d.]+)-([\d.]+)\) us +kernel +([\d.]+) ", line)
            if m:
                B, H, Hkv, S, D = map(int, m.group(1, 2, 3, 4, 5))
                parent, lo, hi, kernel = map(float, m.group(7, 8, 9, 10))
                rows.setdefault((B, H, Hkv, S, S, D), []).append(parent - kernel > hi - lo)
    assert len(rows) >= 6 and all(len(v) == 4 for v in rows.values())
    assert {k for k, v in rows.items() if all(v)} == {k for k, v in attention_route._FP8_GQA_TABLE.items() if v}
    assert not attention_route._fp8_gqa_route_takes(3, 4, 2, 128, 128, 64)


@pytest.mark.parametrize("shape", [(1, 4, 4, 128, 128, 64), (1, 6, 2, 128, 128, 64), (1, 4, 3, 128, 128, 64), (1, 32, 2, 128, 128, 64), (1, 4, 2, 128, 192, 64),
                                   (1, 4, 2, 128, 64, 64), (1, 4, 2, 128, 16512, 64), (1, 4, 2, 128, 128, 32), (1, 4, 2, 128, 128, 96), (65536, 2, 1, 128, 128, 64),
                                   (1, 4, 0, 128, 128, 64)])
def test_shapes_outside_the_contract_are_declined_on_the_host(monkeypatch, shape):
    monkeypatch.setenv("QT_FUSED_ATTENTION", "1")
    assert attention_route._fp8_gqa_core_for(*shape) is None
    assert attention_route._fp8_gqa_core_for(1, 32, 8, 2048, 2048, 128) == "qt_attention_fp8_gqa"
