"""Converted per-tensor int8 convolutions on the device: qt_q8_conv2d (csrc/qt_mx_conv.hip) and qt_quantize_codes_nhwc_*
(csrc/qt_elementwise.hip) through the C ABI, the operator quantized_ops.conv2d_q, its fallbacks, a converted CNN and its graph capture.

Exact tier: random int8 codes.  The reference is the fp64 unfold + matmul on the host (every sum is an integer below 2^53: exact)
followed by the kernel's stated rounding chain in torch on the host: the int32 sum converted to fp32 round-to-nearest-even, + bias in
fp32, rounded to the output dtype (fp32: optionally folded through the identity value map), times the dequantize factor, rounded
again.  The device result must equal it bit for bit.
The codes sit between margins of 0xFF (-1 as a code: a read outside the operand changes a sum), the output between margins of NaN."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from kernel_launch import nv, stream  # noqa: F401

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32

# (N, H, W, Cin, Cout, (kh, kw), stride, padding, dilation)
CASES = {
    "m_under_tile": (1, 5, 5, 32, 8, (3, 3), (1, 1), (1, 1), (1, 1)),        # M = 25; K = 288: two k tiles + a 32 tail, every tile crosses taps
    "k_under_tile": (2, 7, 7, 64, 16, (1, 1), (2, 2), (0, 0), (1, 1)),       # K = 64
    "seven_by_seven": (1, 9, 9, 32, 16, (7, 7), (2, 2), (3, 3), (1, 1)),     # four-tap look-ahead that wraps across filter rows
    "ragged_mn": (2, 19, 19, 96, 136, (3, 3), (2, 2), (2, 1), (2, 2)),       # M = 180, Cout = 136: two ragged tiles each way, dilation
    "one_by_five": (1, 6, 8, 32, 16, (1, 5), (1, 1), (0, 2), (1, 1)),
    "five_by_one": (1, 8, 6, 32, 16, (5, 1), (1, 1), (2, 0), (1, 1)),
    "pm127": (1, 4, 4, 128, 8, (3, 3), (1, 1), (1, 1), (1, 1)),              # |sum| up to 1152 * 16129 > 2^24 (an even number: still exact)
    "pm127_odd": (1, 4, 4, 128, 8, (3, 3), (1, 1), (1, 1), (1, 1)),          # one weight code 126: odd sums above 2^24, int -> fp32 rounds
    "m128": (1, 4, 4, 128, 8, (3, 3), (1, 1), (1, 1), (1, 1)),               # all codes -128: 1152 * 16384 < 2^31, no wrap
}


def geometry(case):
    n, h, w, cin, cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw) = CASES[case]
    return (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def conv_exact(xq, wq, stride, padding, dilation):
    """xq [N, Cin, H, W], wq [Cout, Cin, kh, kw] integer-valued -> the exact sums, fp64 NHWC [N, Ho, Wo, Cout] (unfold + matmul)."""
    n, cout = xq.shape[0], wq.shape[0]
    cols = F.unfold(xq.double(), wq.shape[2:], dilation, padding, stride)               # [N, Cin kh kw, L]
    out = torch.matmul(wq.double().reshape(cout, -1), cols)                             # [N, Cout, L]
    return out.transpose(1, 2).contiguous()                                             # [N, L, Cout]


def fold32(v):
    """The identity value map on an fp32 tensor: the high 16 bits with a sticky bit."""
    pre = v.contiguous().view(torch.int32)
    return ((pre & -65536) | ((pre & 0xFFFF) != 0).int() * 65536).view(torch.float32)


def chain(exact, bias, s, dtype, fold):
    """The rounding chain of the epilogue on the host.  exact fp64 [..., Cout]; bias / s in `dtype` ([Cout] / [1] or [Cout]) or None."""
    v = exact.float()                                             # fp64 holds the integer exactly: this is RNE int -> fp32
    if bias is not None:
        v = v + bias.float()
    if dtype == BF16:
        v = v.bfloat16()
        return (v.float() * s.float()).bfloat16() if s is not None else v
    if fold:
        v = fold32(v)
    return v * s if s is not None else v


@functools.lru_cache(maxsize=None)
def operands(case):
    n, h, w, cin, cout, (kh, kw), stride, padding, dilation = CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    if case.startswith("pm127"):
        sign = (torch.randint(0, 2, (cin,), generator=g) * 2 - 1)
        xq = (127 * sign).view(1, cin, 1, 1).expand(n, cin, h, w).contiguous()
        wsign = torch.tensor([1, -1] * (cout // 2)).view(cout, 1, 1, 1)
        wq = ((127 * sign).view(1, cin, 1, 1) * wsign).expand(cout, cin, kh, kw).contiguous()
        if case == "pm127_odd":
            wq[:, 0, 1, 1] = wq[:, 0, 1, 1] // 127 * 126          # the centre tap: inside every output pixel's window
    elif case == "m128":
        xq = torch.full((n, cin, h, w), -128)
        wq = torch.full((cout, cin, kh, kw), -128)
    else:
        xq = torch.randint(-128, 128, (n, cin, h, w), generator=g)
        wq = torch.randint(-128, 128, (cout, cin, kh, kw), generator=g)
    exact = conv_exact(xq, wq, stride, padding, dilation)
    bias = torch.randint(-3000, 3000, (cout,), generator=g).float()
    scale = torch.rand(cout, generator=g) * 1e-3 + 1e-4
    return dict(x=xq.permute(0, 2, 3, 1).contiguous().to(torch.int8), w=wq.permute(0, 2, 3, 1).contiguous().to(torch.int8),
                exact=exact, bias=bias, scale=scale)


class Margins:
    """A byte array on the device between two margins of `fill`."""
    PAD = 256

    def __init__(self, host, fill=0xFF):
        host = host.contiguous().view(torch.uint8).reshape(-1)
        self.n, self.fill = host.numel(), fill
        self.raw = torch.full((self.n + 2 * self.PAD,), fill, dtype=torch.uint8, device="cuda")
        self.raw[self.PAD:self.PAD + self.n] = host.cuda()
        self.image = self.raw.clone()
        assert (self.raw.data_ptr() + self.PAD) % 16 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.PAD

    def unchanged(self):
        return torch.equal(self.raw, self.image)


def q8_conv(nv, case, ops, dtype, bias, s, per_col, fold):
    """qt_q8_conv2d twice into NaN-filled buffers: status 0, margins intact, both launches the same bits -> y [N, Ho Wo, Cout] (host)."""
    n, h, w, cin, cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw) = CASES[case]
    ho, wo = geometry(case)
    count, pad = n * ho * wo * cout, 64
    xc, wc = Margins(ops["x"]), Margins(ops["w"])
    b = bias.to(dtype).cuda() if bias is not None else None
    sd = s.to(dtype).cuda() if s is not None else None
    runs = []
    for _ in range(2):
        buf = torch.full((count + 2 * pad,), float("nan"), dtype=dtype, device="cuda")
        rc = nv.lib().qt_q8_conv2d(xc.ptr, wc.ptr, buf.data_ptr() + pad * buf.element_size(), int(dtype == F32),
                                   b.data_ptr() if b is not None else None, sd.data_ptr() if sd is not None else None, per_col, fold,
                                   n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, stream())
        assert rc == 0, f"case {case}: status {rc}"
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool(host[:pad].isnan().all()) and bool(host[pad + count:].isnan().all()), f"case {case}: a margin of y was written"
        assert xc.unchanged() and wc.unchanged(), f"case {case}: an operand or its margins changed"
        runs.append(host[pad:pad + count].reshape(n, ho * wo, cout))
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(runs[0].view(bits), runs[1].view(bits)), f"case {case}: two launches differ"
    assert not bool(runs[0].isnan().any()), f"case {case}: an element of y was not written (or a margin was read)"
    return runs[0]


def same_bits(got, want, what):
    bits = torch.int16 if got.dtype == BF16 else torch.int32
    bad = got.contiguous().view(bits) != want.contiguous().view(bits)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}: " \
                                f"{got[bad][0].item()} != {want[bad][0].item()}"


@pytest.mark.parametrize("case", list(CASES))
def test_q8_conv2d_is_exact(nv, case):
    """Bit equality with the exact sums pushed through the stated rounding chain: bare sums, then bias with a per-tensor and a
    per-column factor, bf16 and fp32 outputs, the fp32 identity fold on and off."""
    ops = operands(case)
    exact, bias, scale = ops["exact"], ops["bias"], ops["scale"]
    if case == "pm127":
        assert float(exact.abs().max()) == 1152 * 16129 > 2 ** 24
    if case == "pm127_odd":
        assert float(exact.abs().max()) > 2 ** 24 and bool((exact.float().double() != exact).any())      # the conversion does round
    if case == "m128":
        assert float(exact.max()) == 1152 * 16384
    same_bits(q8_conv(nv, case, ops, F32, None, None, 0, 0), chain(exact, None, None, F32, 0), f"{case} bare fp32")
    same_bits(q8_conv(nv, case, ops, BF16, None, None, 0, 0), chain(exact, None, None, BF16, 0), f"{case} bare bf16")
    for per_col in (0, 1):
        s = scale if per_col else scale[:1].clone()
        for fold in (0, 1):
            same_bits(q8_conv(nv, case, ops, F32, bias, s, per_col, fold), chain(exact, bias, s, F32, fold), f"{case} fp32 {per_col} {fold}")
        b16, s16 = bias.bfloat16(), s.bfloat16()
        same_bits(q8_conv(nv, case, ops, BF16, b16, s16, per_col, 0), chain(exact, b16, s16, BF16, 0), f"{case} bf16 {per_col}")


def _call(nv, x, w, y, geo, dtype=F32, bias=None, s=None):
    n, h, wd, cin, cout, kh, kw = geo
    return nv.lib().qt_q8_conv2d(x, w, y, int(dtype == F32), bias, s, 0, 0, n, h, wd, cin, cout, kh, kw, 1, 1, 0, 0, 1, 1, stream())


def test_q8_conv2d_declines(nv):
    """Cin the tap arithmetic does not cover, a contraction whose int32 sum could wrap, a misaligned pointer: refused before any
    launch; empty outputs are QT_OK without a launch.  The output buffer keeps its sentinel in every case."""
    x = torch.zeros(1 << 20, dtype=torch.int8, device="cuda")
    w = torch.zeros(1 << 20, dtype=torch.int8, device="cuda")
    y = torch.full((4096,), float("nan"), dtype=F32, device="cuda")
    s = torch.ones(64, dtype=F32, device="cuda")
    xp, wp, yp = x.data_ptr(), w.data_ptr(), y.data_ptr()
    for cin in (16, 48):
        assert _call(nv, xp, wp, yp, (1, 4, 4, cin, 8, 1, 1)) == nv.QT_ERR_BAD_ARG, cin
    # kh kw Cin = 2^17 exactly (one output pixel, Cout = 1: both operands fit the buffers) and just below it
    assert _call(nv, xp, wp, yp, (1, 2, 2, 1 << 15, 1, 2, 2)) == nv.QT_ERR_BAD_ARG
    assert _call(nv, xp, wp, yp, (1, 64, 64, 32, 1, 64, 64)) == nv.QT_ERR_BAD_ARG
    for dx, dw_, dy, ds in ((1, 0, 0, 0), (0, 8, 0, 0), (0, 0, 4, 0), (0, 0, 0, 4)):
        assert _call(nv, xp + dx, wp + dw_, yp + dy, (1, 4, 4, 32, 8, 1, 1), s=s.data_ptr() + ds) == nv.QT_ERR_UNALIGNED
    assert _call(nv, xp, wp, yp, (1, 4, 4, 32, 8, 1, 1), bias=s.data_ptr() + 8) == nv.QT_ERR_UNALIGNED
    assert _call(nv, xp, wp, yp, (0, 4, 4, 32, 8, 1, 1)) == 0
    assert _call(nv, xp, wp, yp, (1, 4, 4, 32, 0, 1, 1)) == 0
    assert _call(nv, xp, wp, yp, (1, 2, 2, 32, 8, 3, 3)) == 0              # filter larger than the plane: no output pixel
    torch.cuda.synchronize()
    assert bool(y.isnan().all())


def test_q8_conv2d_largest_contraction_below_the_limit(nv):
    """kh kw Cin = 2^17 - 32 with every code -128: the largest sum the entry point admits, (2^17 - 32) * 2^14 = 4095 * 2^19 < 2^31,
    comes out exact (twelve significant bits: no rounding in the conversion either)."""
    k = (1 << 17) - 32
    cin, kh, kw = k // 9, 3, 3                                    # 14560 = 32 * 455
    assert cin % 32 == 0 and cin * 9 == k
    x = torch.full((1, 3, 3, cin), -128, dtype=torch.int8, device="cuda")
    w = torch.full((8, kh, kw, cin), -128, dtype=torch.int8, device="cuda")
    y = torch.full((8,), float("nan"), dtype=F32, device="cuda")
    assert _call(nv, x.data_ptr(), w.data_ptr(), y.data_ptr(), (1, 3, 3, cin, 8, kh, kw)) == 0
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), torch.full((8,), float(k * 16384), dtype=torch.float64))


# ---- the codes kernel ---------------------------------------------------------------------------------------------------------
def int8_map(device):
    import quantized_training as qt
    return qt.get_quantization_map("int8", torch.device(device))


def documented_codes(q):
    """The narrowing rule of qt_quantize_codes_nhwc_* on mapped values: truncate toward zero, saturate to [-128, 127], NaN -> 0."""
    v = q.float()
    return torch.where(v.isnan(), torch.zeros_like(v), v.trunc().clamp(-128, 127)).to(torch.int8)


def planted(shape, dtype, s, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * 40 * s).to(dtype)
    flat = x.view(-1)
    tiny = 1e-40 if dtype == F32 else 2.0 ** -130                     # subnormal in either dtype
    specials = [0.0, -0.0, tiny, -tiny, 127.4 * s, -128.6 * s, 300 * s, -300 * s, 1e30, -1e30, float("inf"), float("-inf"), float("nan")]
    pos = torch.randperm(flat.numel(), generator=g)[:len(specials) * 3]
    for i, p in enumerate(pos.tolist()):
        flat[p] = specials[i % len(specials)]
    return x


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("c,hw", [(32, (1, 1)), (32, (5, 7)), (32, (8, 8)), (96, (1, 1)), (96, (5, 7)), (96, (8, 8))])
def test_codes_kernel_matches_quantize(nv, dtype, layout, c, hw):
    """One pass from the activation to int8 NHWC codes: bit for bit quantize(x, s, qmap).to(int8) permuted to NHWC where the map
    gives an integer in [-128, 127] (every finite input), the documented code elsewhere; margins of the code buffer intact."""
    from quantized_training import pt2e_native
    s = 0.05
    x = planted((2, c, *hw), dtype, s, c + hw[0] * 100)
    scale = torch.tensor([s]).to(dtype)
    q = torch.ops.quantized_ops.quantize(x, scale, None, None, None, int8_map("cpu"))          # the CPU formulation
    want = documented_codes(q).permute(0, 2, 3, 1).reshape(-1, c)
    ok = q.float().isfinite() & (q.float() == q.float().round()) & (q.float().abs() <= 128)
    assert torch.equal(documented_codes(q)[ok], q.to(torch.int8)[ok])
    assert bool(q.float().isnan().any())                                                      # the NaN rule is exercised
    xd = x.cuda()
    if layout == "channels_last":
        xd = xd.contiguous(memory_format=torch.channels_last)
    n, hw_n = 2, hw[0] * hw[1]
    from quantized_training.mx_conv import _nhwc_strides
    from quantized_training.decomposed import _lut_format
    xs = _nhwc_strides(xd) if layout == "nchw" else (hw_n * c, c, 1)
    out = Margins(torch.zeros(n * hw_n * c, dtype=torch.int8), fill=0xA5)
    out.raw[out.PAD:out.PAD + out.n] = 0x5A
    qmap, sd, fmt = int8_map("cuda"), scale.cuda(), _lut_format()
    fn = nv.lib().qt_quantize_codes_nhwc_bf16 if dtype == BF16 else nv.lib().qt_quantize_codes_nhwc_f32
    assert fn(xd.data_ptr(), out.ptr, n, hw_n, c, *xs, ctypes.byref(fmt), qmap.data_ptr(), sd.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    raw = out.raw.cpu()
    assert bool((raw[:out.PAD] == 0xA5).all()) and bool((raw[out.PAD + out.n:] == 0xA5).all()), "a margin of the codes was written"
    got = raw[out.PAD:out.PAD + out.n].view(torch.int8).reshape(-1, c)
    assert torch.equal(got, want), f"{int((got != want).sum())} codes differ"
    # and through the package helper, which picks the strides itself
    got2 = pt2e_native.conv_codes_nhwc(xd, sd, qmap)
    assert torch.equal(got2.cpu(), want)
    # against the device's own quantize (the same device function): equal wherever it yields an int8 integer
    qd = torch.ops.quantized_ops.quantize(xd, sd, None, None, None, qmap).cpu()
    assert torch.equal(documented_codes(qd).permute(0, 2, 3, 1).reshape(-1, c), want)


def test_codes_kernel_declines(nv):
    from quantized_training.decomposed import _lut_format
    x = torch.zeros(2 * 24 * 16 + 8, dtype=BF16, device="cuda")
    out = torch.full((2 * 24 * 16 + 16,), 0x5A, dtype=torch.int8, device="cuda")
    qmap, s, fmt = int8_map("cuda"), torch.ones(1, dtype=BF16, device="cuda"), _lut_format()
    fn = nv.lib().qt_quantize_codes_nhwc_bf16

    def call(xp, op, n, hw, c, strides, lut=qmap.data_ptr()):
        return fn(xp, op, n, hw, c, *strides, ctypes.byref(fmt), lut, s.data_ptr(), stream())
    assert call(x.data_ptr(), out.data_ptr(), 2, 16, 24, (384, 1, 16)) == nv.QT_ERR_BAD_ARG           # C % 16
    assert call(x.data_ptr(), out.data_ptr(), 2, 16, 16, (512, 1, 16)) == nv.QT_ERR_BAD_ARG           # not one of the two layouts
    assert call(x.data_ptr(), out.data_ptr(), 2, 16, 16, (256, 1, 16), lut=None) == nv.QT_ERR_BAD_ARG
    assert call(x.data_ptr() + 2, out.data_ptr(), 2, 16, 16, (256, 1, 16)) == nv.QT_ERR_UNALIGNED
    assert call(x.data_ptr(), out.data_ptr() + 1, 2, 16, 16, (256, 1, 16)) == nv.QT_ERR_UNALIGNED
    assert call(x.data_ptr(), out.data_ptr(), 0, 16, 16, (256, 1, 16)) == 0
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())


# ---- the operator ---------------------------------------------------------------------------------------------------------------
def op_args(dtype, n=2, cin=32, h=9, w=7, cout=24, k=(3, 3), per_channel=False, bias=True, seed=0, scale_dtype=None, groups=1):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, cin, h, w, generator=g) * 2).to(dtype).cuda()
    scale = torch.tensor(0.04).to(scale_dtype or dtype).cuda()
    wc = torch.randint(-127, 128, (cout, *k, cin // groups), generator=g).to(torch.int8).cuda()
    b = torch.randint(-4000, 4000, (cout,), generator=g).to(dtype).cuda() if bias else None
    out_scale = (torch.rand(cout, 1, 1, generator=g) * 1e-3 + 1e-4 if per_channel else torch.tensor([3e-4])).to(dtype).cuda()
    return x, scale, int8_map("cuda"), wc, b, out_scale


def unfused(x, scale, qmap, wc, b, stride, padding, dilation, groups, out_scale, out_map):
    """The three nodes of the parent graph on the tensors it stored: the weight as [Cout, Cin, kh, kw] values."""
    xq = torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap)
    y = F.conv2d(xq, wc.permute(0, 3, 1, 2).to(x.dtype).contiguous(), b, stride, padding, dilation, groups)
    return torch.ops.quantized_ops.dequantize(y, out_scale, None, None, None, out_map)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_operator_equals_the_exact_reference(nv, monkeypatch, dtype, per_channel, layout):
    """conv2d_q on the device against the exact-tier reference built from its own arguments: the codes the quantize op yields, the
    exact sums, the rounding chain.  channels_last result of the logical shape; counted in STATS."""
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    x, scale, qmap, wc, b, out_scale = op_args(dtype, per_channel=per_channel)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    stride, padding, dilation = [2, 1], [1, 2], [1, 2]
    ident = int8_map("cuda").new_empty(0)           # any tensor: the identity map's content is not read by the native route
    before = pt2e_native.STATS["conv2d_int8"]
    for out_map in (None, ident):
        y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, wc, b, stride, padding, dilation, 1, out_scale, out_map, "int8")
        assert y.shape == (2, 24, 5, 7) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
        xq = torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap).cpu()
        exact = conv_exact(xq, wc.cpu().permute(0, 3, 1, 2), stride, padding, dilation)
        want = chain(exact, b.cpu(), out_scale.cpu().reshape(-1), dtype, int(out_map is not None))
        same_bits(y.permute(0, 2, 3, 1).reshape(2, -1, 24).cpu(), want, f"conv2d_q {dtype} {layout}")
    assert pt2e_native.STATS["conv2d_int8"] - before == 2


FALLBACKS = {
    "groups": dict(groups=2, cin=64),
    "cin_48": dict(cin=48),
    "stem": dict(cin=3),
    "fp16": dict(dtype=torch.float16),
    "float_map": dict(scale_dtype=F32, qmap="float"),
    "misaligned": dict(offset=1),
    "route_rule": dict(rule=lambda *a: False),
}


@pytest.mark.parametrize("which", list(FALLBACKS))
def test_operator_fallbacks_equal_the_unfused_graph(nv, monkeypatch, which):
    """Everything the kernels do not take runs quantize -> aten.conv2d -> dequantize verbatim: the same bits as those three nodes on
    the same device, no native launch counted, and the reason recorded."""
    from quantized_training import pt2e_native
    cfg = dict(FALLBACKS[which])
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", "rule" in cfg)
    if "rule" in cfg:
        monkeypatch.setattr(pt2e_native, "_conv_q_route_takes", cfg.pop("rule"))
    dtype, offset, qm = cfg.pop("dtype", BF16), cfg.pop("offset", 0), cfg.pop("qmap", None)
    groups = cfg.get("groups", 1)
    x, scale, qmap, wc, b, out_scale = op_args(dtype, **cfg)
    if qm == "float":
        qmap = qmap.float()
    if offset:
        base = torch.zeros(x.numel() + 8, dtype=dtype, device="cuda")
        base[offset:offset + x.numel()] = x.reshape(-1)
        x = base[offset:offset + x.numel()].view(x.shape)
        assert x.data_ptr() % 16 != 0
    before, reasons = pt2e_native.STATS["conv2d_int8"], sum(pt2e_native.CONV_Q_REASONS.values())
    y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, wc, b, [1, 1], [1, 1], [1, 1], groups, out_scale, None, "int8")
    want = unfused(x, scale, qmap, wc, b, [1, 1], [1, 1], [1, 1], groups, out_scale, None)
    assert pt2e_native.STATS["conv2d_int8"] == before and sum(pt2e_native.CONV_Q_REASONS.values()) == reasons + 1
    assert y.dtype == want.dtype and y.shape == want.shape
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


# ---- a converted CNN --------------------------------------------------------------------------------------------------------------
class SmallCnn(torch.nn.Module):
    """A stem over 3 channels (stays aten.conv2d), two 3 x 3 convolutions at 32 / 64 channels, a residual add, a Linear head."""

    def __init__(self):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, 32, 3, padding=1)
        self.c1 = torch.nn.Conv2d(32, 64, 3, padding=1, stride=2)
        self.c2 = torch.nn.Conv2d(64, 64, 3, padding=1)
        self.fc = torch.nn.Linear(64, 10)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        x = torch.relu(self.c1(x))
        x = torch.relu(self.c2(x)) + x
        return self.fc(x.mean((2, 3)))


def converted(native, monkeypatch, device="cuda"):
    from quantized_training import quantize_pt2e as qp
    monkeypatch.setenv("QT_PT2E_NATIVE", native)
    torch.manual_seed(3)
    x = torch.randn(4, 3, 14, 14).bfloat16().to(device)
    torch.manual_seed(4)
    net = SmallCnn().to(device).bfloat16().eval()
    spec = "int8,qs=per_tensor_symmetric"
    gm = qp.prepare_pt2e(net, qp.get_default_quantizer(spec, None, spec, "int24"), (x,))
    with torch.no_grad():
        gm(x), gm(x * 0.5)
    return qp.convert_pt2e(gm), x


def targets(gm):
    return [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]


def ulp(v, dtype):
    """One rounding step of `dtype` at magnitude v (fp64 tensor)."""
    mant = 7 if dtype == BF16 else 23
    e = torch.floor(torch.log2(v.clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def layer_bound(xq, wc, b, out_scale, stride, padding, dilation, dtype):
    """Per element: the fp32 accumulation of the value-tensor convolution is within K 2^-24 sum|q_x||q_w| of the exact sum; one
    rounding step of the output dtype at each of the two rounding points (the convolution's output, the dequantize product); scaled
    by |s|.  Returns (exact result in fp64 [N, L, Cout], bound)."""
    k = wc.shape[1] * wc.shape[2] * wc.shape[3]
    w = wc.cpu().permute(0, 3, 1, 2)
    exact = conv_exact(xq, w, stride, padding, dilation)
    acc = k * 2.0 ** -24 * conv_exact(xq.abs(), w.abs(), stride, padding, dilation)
    v = exact + (b.cpu().double() if b is not None else 0.0)
    s = out_scale.cpu().double().reshape(-1).abs()
    # the first rounding point: a library convolution may round the sum before it adds the bias and round again behind the add --
    # two half steps, one at |sum| and one at |sum + bias|: one step at the larger magnitude covers both
    first = acc + ulp(torch.maximum(exact.abs(), v.abs()) + acc, dtype)
    return v * out_scale.cpu().double().reshape(-1), first * s + ulp((v.abs() + first) * s, dtype)


def test_converted_cnn_runs_conv2d_q(nv, monkeypatch):
    """Device conversion with QT_PT2E_NATIVE=1: both eligible convolutions and the Linear are native nodes, the stem stays
    aten.conv2d; with =0 the graph is upstream's.  STATS counts one launch per eligible layer.  Layer by layer, on the same input,
    |native node - three nodes of the =0 graph| <= the derived bound per element, for the three nodes run on the device, on the host
    in bf16, and (convolution and dequantize, on the same codes) on the host in fp32.  The comparison is per layer because the
    requantization between layers is discontinuous: an end-to-end bound per element does not exist."""
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    g0, x = converted("0", monkeypatch)
    g1, _ = converted("1", monkeypatch)
    t0, t1 = targets(g0), targets(g1)
    assert t0.count("aten.conv2d.default") == 3 and not any("conv2d_q" in t for t in t0) and not any("linear_q" in t for t in t0)
    assert t1.count("aten.conv2d.default") == 1 and t1.count("quantized_ops.conv2d_q.default") == 2
    assert t1.count("quantized_ops.linear_q.default") == 1 and t1.count("aten.linear.default") == 0
    for name in ("c1_weight_codes", "c2_weight_codes"):
        assert getattr(g1, name).dtype == torch.int8
    assert tuple(g1.c1_weight_codes.shape) == (64, 3, 3, 32) and tuple(g1.c2_weight_codes.shape) == (64, 3, 3, 64)

    before = dict(pt2e_native.STATS)
    with torch.no_grad():
        y0 = g0(x)
    assert {k: pt2e_native.STATS[k] - before[k] for k in before} == {k: 0 for k in before}
    with torch.no_grad():
        y1 = g1(x)
    ran = {k: pt2e_native.STATS[k] - before[k] for k in before}
    assert ran["conv2d_int8"] == 2 and ran["linear_int8"] == 1, ran
    assert y1.shape == y0.shape and bool(y1.float().isfinite().all())

    checked = []

    class PerLayer(torch.fx.Interpreter):
        def call_function(self, target, args, kwargs):
            out = super().call_function(target, args, kwargs)
            if target == torch.ops.quantized_ops.conv2d_q.default:
                inp, scale, qmap, wc, b, stride, padding, dilation, groups, out_scale, out_map, _ = args
                xq = torch.ops.quantized_ops.quantize(inp, scale, None, None, None, qmap)
                _, bound = layer_bound(xq.cpu(), wc, b, out_scale, stride, padding, dilation, inp.dtype)
                dev = unfused(inp, scale, qmap, wc, b, stride, padding, dilation, groups, out_scale, out_map)
                host = unfused(inp.cpu(), scale.cpu(), qmap.cpu(), wc.cpu(), b.cpu(), stride, padding, dilation, groups, out_scale.cpu(),
                               out_map.cpu() if out_map is not None else None)
                rows = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).double().cpu()
                small = float(conv_exact(xq.cpu().abs(), wc.cpu().permute(0, 3, 1, 2).abs(), stride, padding, dilation).max()) < 2 ** 24
                equal = torch.equal(out.view(torch.int16), dev.contiguous(memory_format=torch.channels_last).view(torch.int16))
                print(f"conv2d_q {tuple(wc.shape)}: sum|q_x||q_w| < 2^24 everywhere: {small}; native and value-tensor routes "
                      f"bit-equal: {equal}")
                # the fp32 run of the convolution and the dequantize on the host, on the codes the model's own quantize node produced
                # (quantize itself is not rerun in fp32: x / s in fp32 indexes the value map through the folded image and yields
                # other codes, i.e. another problem); its rounding points are fp32's, far inside the bf16 steps of the bound
                host32 = F.conv2d(xq.cpu().float(), wc.cpu().permute(0, 3, 1, 2).float().contiguous(), b.cpu().float(), stride, padding,
                                  dilation, groups) * out_scale.cpu().float()
                for other, what in ((dev, "device graph"), (host, "host graph in bf16"), (host32, "host graph in fp32")):
                    diff = (rows(out) - rows(other)).abs()
                    print(f"conv2d_q {tuple(wc.shape)}: worst |native - {what}| / bound = {float((diff / bound).max()):.3f}")
                    assert bool((diff <= bound).all()), f"native vs the {what}, layer {tuple(wc.shape)}: worst " \
                                                        f"{float((diff / bound).max()):.3f} of the bound"
                checked.append(tuple(wc.shape))
            return out

    with torch.no_grad():
        PerLayer(g1).run(x)
    assert checked == [(64, 3, 3, 32), (64, 3, 3, 64)]


def test_converted_cnn_default_rule_counts_what_it_takes(nv, monkeypatch):
    """Under the committed route rule the count of native launches is the number of layers the rule lists; the rest run the three
    nodes and the result has the same shape and dtype."""
    from quantized_training import pt2e_native
    g1, x = converted("1", monkeypatch)
    n = x.shape[0]
    takes = sum(bool(pt2e_native._conv_q_route_takes(n * 7 * 7, 64, cin, 3, 3)) for cin in (32, 64))
    before = pt2e_native.STATS["conv2d_int8"]
    with torch.no_grad():
        y = g1(x)
    assert pt2e_native.STATS["conv2d_int8"] - before == takes
    assert y.shape == (4, 10) and y.dtype == BF16


def test_converted_cnn_graph_capture(nv, monkeypatch):
    """A torch.cuda.graph replay of the converted model equals the eager call bit for bit, and so do two eager calls."""
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    g1, x = converted("1", monkeypatch)
    with torch.no_grad():
        e1 = g1(x).clone()
        e2 = g1(x).clone()
    assert torch.equal(e1.view(torch.int16), e2.view(torch.int16))
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        g1(static_x)                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    before = pt2e_native.STATS["conv2d_int8"]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = g1(static_x)
    assert pt2e_native.STATS["conv2d_int8"] - before == 2          # the capture took the native route
    static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), e1.view(torch.int16))
