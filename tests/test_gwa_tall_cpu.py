"""qt_linear_gwa_tall_bf16 without a GPU: its symbols, its plan, its host-side refusals and the committed route rule."""
import ctypes
import os
import re

import pytest

from quantized_training import _native, pt2e_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256                                              # what the library assumes where no device answers


def test_entry_points_are_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(ROOT, "include", "qt_hip.h")).read()
    assert "#define QT_ABI_VERSION 3" in header
    cdll = ctypes.CDLL(_native.LIB_PATH)
    for name in ("qt_linear_gwa_tall_plan", "qt_linear_gwa_tall_bf16"):
        decl = re.search(r"\bint\s+" + name + r"\(([^;]*?)\);", header, re.S)
        assert decl is not None and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
        getattr(cdll, name)
    assert "csrc/qt_gwa_tall.hip" in header and "in split order" in header


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("tile_m", [0, 128, 256])
def test_plan_is_a_fixed_function_within_its_constraints(bits, tile_m):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else CUS
    for M in (1, 33, 128, 129, 256, 1024, 4096):
        for N in (8, 128, 136, 4096, 11008):
            for K in (32, 96, 256, 4096, 11008 // 32 * 32):
                bm, ks, wbytes, ntick = _native.gwa_tall_plan(M, N, K, bits, tile_m)
                tiles = -(-M // bm) * -(-N // 128)
                nss = -(-K // (128 if bits == 4 else 64))
                assert bm in (128, 256) and (tile_m == 0 or bm == tile_m) and ks in (1, 2, 4, 8)
                assert ks == 1 or (tiles * ks <= cus and nss // ks >= 2), (M, N, K, bm, ks)
                assert (wbytes, ntick) == ((tiles * ks * bm * 128 * 4, tiles) if ks > 1 else (0, 0))
    assert _native.gwa_tall_plan(128, 4096, 4096, 4)[:2] == (128, 8) or cus != CUS          # 32 tiles on 256 CUs
    assert _native.gwa_tall_plan(64, 16, 128, 3) is None and _native.gwa_tall_plan(64, 12, 128, 4) is None and _native.gwa_tall_plan(64, 16, 128, 4, 64) is None


def test_host_side_refusals_need_no_device():
    L, BAD, UNAL = _native.lib(), _native.QT_ERR_BAD_ARG, _native.QT_ERR_UNALIGNED
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    p += (-p) % 16

    def call(x=p, M=256, N=128, K=1024, bs=128, bits=4, tile=128, split=2, ws=p, ws_bytes=1 << 30, tickets=p, n_tickets=1 << 20):
        return L.qt_linear_gwa_tall_bf16(x, p, p, p, None, p, M, N, K, bs, bits, 0.0, tile, split, ws, ws_bytes, tickets, n_tickets, None)
    assert [call(x=None), call(bits=3), call(bs=48), call(M=-1), call(tile=64), call(tile=16), call(split=3), call(split=16)] == [BAD] * 8
    assert [call(ws=None), call(tickets=None), call(ws_bytes=2 * 2 * 128 * 128 * 4 - 1), call(n_tickets=1)] == [BAD] * 4
    assert [call(K=144), call(N=12), call(x=p + 2), call(ws=p + 4), call(tickets=p + 2), call(K=64)] == [UNAL] * 6
    assert call(M=0) == 0 and call(M=0, ws=None, tickets=None) == 0


def test_route_rules_agree_with_the_committed_measurement():
    rows = [ln for ln in open(os.path.join(ROOT, "profiles", "gwa_tall.txt")) if ln.startswith("uint")]
    assert len(rows) >= 4 * 6
    clears = {}
    for ln in rows:
        m = re.match(r"uint(\d) \|\s*(\d+) x\s*(\d+) x\s*(\d+) \|.*\(t\) max < \(b\) min: (yes|no)\s*\| rule -> (tall|gwa_dequantize) ", ln)
        bits, M, N, K = (int(v) for v in m.groups()[:4])
        clears.setdefault((bits, M), []).append(m.group(5) == "yes")
        assert pt2e_native._gwa_tall_route_takes(M, N, K, bits) == (m.group(6) == "tall"), ln
    for (bits, M), won in clears.items():                                      # a class is in the rule only where every weight cleared the bar
        assert all(won) or not any(pt2e_native._gwa_tall_route_takes(M, n, k, bits) for n, k in ((4096, 4096), (11008, 4096), (4096, 11008)))
    # unmeasured: small N K, M just above 32; and the old rule is what it was
    assert not any(pt2e_native._gwa_tall_route_takes(M, 136, 512, 4) for M in (33, 64, 128, 1024))
    assert not pt2e_native._gwa_tall_route_takes(33, 4096, 4096, 4)
    assert [pt2e_native._gwa_route_takes(M, 4096, 4096) for M in (1, 32, 33)] == [True, True, False] and pt2e_native._GWA_FUSED_MAX_M == 32
