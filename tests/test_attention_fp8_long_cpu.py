"""qt_attention_fp8_long without a GPU: declared, bound and built; host-side refusals; the route rule against profiles/attention_fp8_long.txt."""
import ctypes
import os
import re

import pytest

from quantized_training import _native, attention_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK_ARGS = dict(q=4096, k=4096, vt=4096, fmt=0, out=4096, out8=8192, B=1, H=2, Sq=65, Sk=1152, D=128)


def _call(**kw):
    a = dict(OK_ARGS, **kw)
    f8 = _native.format_for("e4m3")
    return _native.lib().qt_attention_fp8_long(a["q"], a["k"], a["vt"], a["fmt"], None, 0, 0, 0, None, 0, 0, 0, 0, None, a["out"], a["out8"], ctypes.byref(f8),
                                               a["B"], a["H"], a["Sq"], a["Sk"], a["D"], 0.125, None)


def test_symbol_is_declared_bound_and_built():
    with open(os.path.join(ROOT, "include", "qt_hip.h")) as f:
        decl = re.search(r"int qt_attention_fp8_long\(([^;]*)\);", f.read())
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(_native.SIGNATURES["qt_attention_fp8_long"][1]) == len(_native.SIGNATURES["qt_attention_fp8"][1])
    assert hasattr(_native.lib(), "qt_attention_fp8_long") and _native.lib().qt_abi_version() == 3


@pytest.mark.parametrize("kw", [dict(Sk=64), dict(Sk=1152 + 64), dict(Sk=16512), dict(D=32), dict(out=None, out8=None), dict(out=4104), dict(out8=8200),
                                dict(B=65536, H=1), dict(fmt=2), dict(q=None)], ids=str)
def test_host_side_refusals(kw):
    """Refused before anything is launched (the pointers are never dereferenced on the host); an empty problem is fine."""
    assert _call(**kw) != 0 and _call(B=0) == 0


def test_the_rule_agrees_with_the_committed_table():
    """Every row of profiles/attention_fp8_long.txt: the rule takes the class exactly when the kernel's median beats the chain's by more
    than the chain's min-max spread, eager and replayed."""
    rows = {}
    with open(os.path.join(ROOT, "profiles", "attention_fp8_long.txt")) as f:
        for line in f:
            m = re.match(r"B (\d+) H (\d+) S (\d+) D (\d+) \S+ +(eager|graph) +chain +([\d.]+) \(([\d.]+)-([\d.]+)\) us +kernel +([\d.]+) ", line)
            if m:
                B, H, S, D = map(int, m.group(1, 2, 3, 4))
                chain, lo, hi, kernel = map(float, m.group(6, 7, 8, 9))
                rows.setdefault((B, H, S, S, D), []).append(chain - kernel > hi - lo)
    assert rows and all(len(v) == 2 for v in rows.values())
    for key, wins in rows.items():
        assert attention_route._fp8_long_route_takes(*key) == all(wins), key
    assert set(k for k, v in attention_route._FP8_LONG_TABLE.items() if v) <= set(rows)
    assert not attention_route._fp8_long_route_takes(1, 2, 1152, 1152, 64)          # a shape nobody measured stays on the chain
