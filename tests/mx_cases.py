"""What the microscaling kernel tests share (tests/test_gpu_mx_strided.py: blocks along an axis that is not the last;
tests/test_gpu_mx_last_axis.py: blocks along the last axis): bit patterns with canonical NaNs, the launch formats, the CPU composite and
the numpy oracle as expectations, and the expectation of the packed operand with its flush rule.  A plain module, imported by name;
it holds no tests."""
import numpy as np
import torch

from oracle import qt_oracle as o

BF16, F32 = torch.bfloat16, torch.float32
IO_IDS = {BF16: "bf16", F32: "f32"}
BITS = {"fp8_e4m3": 8, "fp8_e5m2": 8, "fp6_e2m3": 6, "fp6_e3m2": 6, "fp4_e2m1": 4}


def bits_of(t):
    """tensor (any device) -> canonical bit patterns on the host"""
    t = t.detach().cpu().contiguous()
    if t.dtype == BF16:
        return o.canon_nan16(t.view(torch.int16).numpy().view(np.uint16))
    return o.canon_nan32(t.view(torch.int32).numpy().view(np.uint32))


def canon(a):
    return o.canon_nan16(a) if a.dtype == np.uint16 else o.canon_nan32(a)


def assert_same(got, want, what):
    got, want = got.reshape(-1), want.reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[:4]}: got {got[bad[:4]]} expected {want[bad[:4]]}"


def maps_for(nv, name, row_form):
    """(host map, device map, the qt_format of the launch).  row_form: the row words behind the device map (qt_format.p1 bit 0)."""
    from quantized_training.fake_quantize import _launch_format, get_quantization_map
    host, devm = get_quantization_map(name, "cpu"), get_quantization_map(name, "cuda")
    fmt = nv.QtFormat(nv.QT_FMT_LUT, 0, 0, 0.0, 0.0)
    if row_form:
        fmt = _launch_format(fmt, devm)
        assert fmt.p1 & 1, f"{name}: the device map carries no row form"
    return host, devm, fmt


def qmax_of(name):
    from quantized_training.quantizer.quantizer import get_quant_min_max
    return float(get_quant_min_max(name)[1])


def cpu_pair(x, ax, bs, host_map, qmax, pow2, smap=None):
    s = torch.ops.quantized_ops.calculate_mx_qparam(x, [ax], bs, qmax, pow2, smap)
    q = torch.ops.quantized_ops.quantize(x, s, None, [ax], bs, host_map)
    return s, q


def oracle_fake_quant(x, ax, bs, name, qmax, pow2, smap_name=None):
    xf = x.float().numpy()
    y, s = o.mx_fake_quant(xf, x.dtype == BF16, o.get_quantization_map(name), ax, bs, qmax, pow2,
                           o.get_quantization_map(smap_name) if smap_name else None)
    if x.dtype == BF16:
        return o.canon_nan16(o.f32_to_bf16(y).reshape(y.shape)), o.canon_nan16(o.f32_to_bf16(s).reshape(s.shape))
    return o.canon_nan32(np.ascontiguousarray(y, np.float32).view(np.uint32)), o.canon_nan32(np.ascontiguousarray(s, np.float32).view(np.uint32))


def expected_pack_rows(qt, st, name, bs):
    """qt [rows, K] element values, st [rows, K / bs] scales, both float64, one code row each -> (codes, e8m0, rows compared, blocks
    flushed).  Rows whose values and scales are finite; a block whose scale is below 2^-127 is flushed: codes 0 and byte 0, which is
    what mx_pack makes of zeros at scale 2^-127."""
    rows = np.flatnonzero(np.isfinite(qt).all(axis=1) & np.isfinite(st).all(axis=1))
    qt, st = qt[rows].copy(), st[rows].copy()
    flushed = st < 2.0 ** -127
    qt[np.repeat(flushed, bs, axis=1)] = 0.0
    st[flushed] = 2.0 ** -127
    codes, e8 = o.mx_pack(qt, st, name, bs)
    return codes, e8, rows, int(flushed.sum())


def expected_pack(s_ref, q_ref, name, bs):
    """The packed operand of q [B, K, N] with blocks along K: one code row per column (see expected_pack_rows)."""
    B, K, N = q_ref.shape
    qt = q_ref.float().transpose(1, 2).reshape(B * N, K).numpy().astype(np.float64)
    st = s_ref.float().transpose(1, 2).reshape(B * N, K // bs).numpy().astype(np.float64)
    return expected_pack_rows(qt, st, name, bs)


def f32_binade_patterns():
    """fp32 amax patterns that cross every binade -> (normal, subnormal) uint32 arrays.  Normal: the exponent fields 1 .. 254 with
    mantissa 0 and the 128 highest mantissas (the logarithm reaches the next integer only from within 2^-16 of it:
    csrc/qt_mx_log2_tables.h holds no threshold below 0x7FFFA8).  Subnormal: 2^p + k for p = 0 .. 22, every k up to p = 7, else the 4
    lowest and the 128 highest."""
    mant = np.concatenate([[0], np.arange((1 << 23) - 128, 1 << 23)]).astype(np.uint32)
    normal = ((np.arange(1, 255, dtype=np.uint32) << 23)[:, None] | mant[None, :]).reshape(-1)
    sub = []
    for p in range(23):
        ks = np.arange(1 << p) if p <= 7 else np.concatenate([np.arange(4), np.arange((1 << p) - 128, 1 << p)])
        sub.append((1 << p) + ks)
    return normal, np.concatenate(sub).astype(np.uint32)


def unpack_codes(codes, bits):
    """[rows, K bits / 8] bytes -> [rows, K] element codes (element i in bits [i bits, (i + 1) bits) of the row, little-endian)"""
    b = np.unpackbits(np.ascontiguousarray(codes), axis=1, bitorder="little")
    b = b.reshape(codes.shape[0], -1, bits).astype(np.uint32)
    return (b << np.arange(bits, dtype=np.uint32)).sum(axis=-1)
