"""csrc/qt_mx_log2_tables.h against this machine's torch: the thresholds from which torch.floor(torch.log2(x)), evaluated in the tensor's
dtype, reaches the next integer.  floor_log2_dtype (csrc/qt_mx.h) is restated here on the parsed tables and compared with torch's CPU
result at every positive finite bf16 pattern, subnormals included, and at fp32 patterns that cross every binade
(mx_cases.f32_binade_patterns, the patterns of tests/test_gpu_mx_last_axis.py::test_every_f32_binade).

With the device sweeps this separates two causes: a sweep that fails while this passes is a kernel error; if both fail, this torch
evaluates log2 differently from the one tools/gen_mx_log2_tables.py ran under."""
import os
import re

import numpy as np
import torch

from mx_cases import f32_binade_patterns

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quantized-training_amd", "csrc", "qt_mx_log2_tables.h")


def parse_tables():
    src = open(HEADER).read()
    lo = int(re.search(r"constexpr int kMxLog2Lo = (-?\d+);", src).group(1))
    out = {}
    for name in ("kMxLog2ThrBf16", "kMxLog2ThrF32"):
        m = re.search(name + r"\[(\d+)\] = \{(.*?)\};", src, re.S)
        vals = np.array([int(v, 16) for v in re.findall(r"0x([0-9A-Fa-f]+)u", m.group(2))], dtype=np.int64)
        assert len(vals) == int(m.group(1)) == 128 - lo + 1, name
        out[name] = vals
    return lo, out["kMxLog2ThrBf16"], out["kMxLog2ThrF32"]


def floor_log2_by_table(au, thr, lo):
    """floor_log2_dtype of csrc/qt_mx.h on fp32 bit images (positive, finite, not zero)."""
    au = au.astype(np.int64)
    E, M = au >> 23, au & 0x7FFFFF
    p = np.floor(np.log2(np.maximum(M, 1).astype(np.float64))).astype(np.int64)        # 31 - clz(M): exact, M < 2^23
    e = np.where(E != 0, E - 127, p - 149)
    mn = np.where(E != 0, M, (M << (23 - p)) & 0x7FFFFF)
    return e + (mn >= thr[e + 1 - lo])


def report(au, got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} patterns differ from torch.floor(torch.log2(x)), first "
                           + ", ".join(f"0x{int(au[i]):08X}: table {int(got[i])} torch {int(want[i])}" for i in bad[:8]))


def test_tables_parse_and_hold_23_bit_thresholds():
    lo, b, f = parse_tables()
    assert lo == -148
    for t in (b, f):
        assert ((t >= 0) & (t <= 0x800000)).all()


def test_bf16_table_equals_torch_at_every_positive_finite_pattern():
    lo, thr, _ = parse_tables()
    pats = np.arange(1, 0x7F80, dtype=np.uint16)
    x = torch.from_numpy(pats.view(np.int16)).view(torch.bfloat16)
    want = torch.floor(torch.log2(x)).float().numpy().astype(np.int64)
    report(pats.astype(np.uint32) << 16, floor_log2_by_table(pats.astype(np.uint32) << 16, thr, lo), want, "bf16")


def test_f32_table_equals_torch_across_every_binade():
    lo, _, thr = parse_tables()
    normal, sub = f32_binade_patterns()
    assert len(sub) == 2235 and len(normal) == 254 * 129
    for what, pats in (("fp32 normal", normal), ("fp32 subnormal", sub)):
        x = torch.from_numpy(pats.view(np.int32)).view(torch.float32)
        want = torch.floor(torch.log2(x)).numpy().astype(np.int64)
        got = floor_log2_by_table(pats, thr, lo)
        report(pats, got, want, what)
        # torch's vectorised log2 and its one-element evaluation agree where the result rounds up, so the reference is self-consistent
        up = np.flatnonzero(got != np.where(pats >> 23 != 0, (pats >> 23).astype(np.int64) - 127,
                                            np.floor(np.log2(np.maximum(pats & 0x7FFFFF, 1).astype(np.float64))).astype(np.int64) - 149))
        for i in up[:: max(1, len(up) // 64)]:
            assert int(torch.floor(torch.log2(x[i:i + 1]))) == int(want[i]), f"{what}: 0x{int(pats[i]):08X} alone"
        print(f"[log2 tables] {what}: {len(pats)} patterns, {len(up)} round up")
