"""Converted per-tensor int8 depthwise and narrow pointwise convolutions on the device: qt_q8_dwconv2d (csrc/qt_mx_conv.hip) through the C ABI,
the operator quantized_ops.conv2d_q on its depthwise and pointwise routes, its fallbacks, a converted inverted-residual block and its
graph capture.  The method is that of tests/test_gpu_conv_q.py.

Exact tier: random int8 codes.  The reference is the fp64 grouped convolution on the host (every sum is an integer below 2^24: exact)
followed by the kernel's stated rounding chain in torch on the host; the device result must equal it bit for bit.  The codes sit
between margins of 0xFF (-1 as a code: a read outside the operand changes a sum), the output between margins of NaN."""
import pytest
import torch
import torch.nn.functional as F

import conv_q_depthwise_cases as K
from conv_q_depthwise_cases import BF16, F32
from kernel_launch import nv, stream  # noqa: F401

pytestmark = pytest.mark.gpu


class Margins:
    """A byte array on the device between two margins of `fill`."""
    PAD = 256

    def __init__(self, host, fill=0xFF):
        host = host.contiguous().view(torch.uint8).reshape(-1)
        self.n = host.numel()
        self.raw = torch.full((self.n + 2 * self.PAD,), fill, dtype=torch.uint8, device="cuda")
        self.raw[self.PAD:self.PAD + self.n] = host.cuda()
        self.image = self.raw.clone()
        assert (self.raw.data_ptr() + self.PAD) % 16 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.PAD

    def unchanged(self):
        return torch.equal(self.raw, self.image)


def q8_dwconv(nv, case, ops, dtype, bias, s, per_col, fold):
    """qt_q8_dwconv2d twice into NaN-filled buffers: status 0, margins intact, both launches the same bits -> y [N, Ho Wo, C] (host)."""
    n, h, w, c, (kh, kw), (sh, sw), (ph, pw), (dh, dw) = K.CASES[case]
    ho, wo = K.out_hw(case)
    count, pad = n * ho * wo * c, 64
    xc, wc = Margins(ops["x"]), Margins(ops["w"])
    b = bias.to(dtype).cuda() if bias is not None else None
    sd = s.to(dtype).cuda() if s is not None else None
    runs = []
    for _ in range(2):
        buf = torch.full((count + 2 * pad,), float("nan"), dtype=dtype, device="cuda")
        rc = nv.lib().qt_q8_dwconv2d(xc.ptr, wc.ptr, buf.data_ptr() + pad * buf.element_size(), int(dtype == F32),
                                     b.data_ptr() if b is not None else None, sd.data_ptr() if sd is not None else None, per_col, fold,
                                     n, h, w, c, kh, kw, sh, sw, ph, pw, dh, dw, stream())
        assert rc == 0, f"case {case}: status {rc}"
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool(host[:pad].isnan().all()) and bool(host[pad + count:].isnan().all()), f"case {case}: a margin of y was written"
        assert xc.unchanged() and wc.unchanged(), f"case {case}: an operand or its margins changed"
        runs.append(host[pad:pad + count].reshape(n, ho * wo, c))
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(runs[0].view(bits), runs[1].view(bits)), f"case {case}: two launches differ"
    assert not bool(runs[0].isnan().any()), f"case {case}: an element of y was not written (or a margin was read)"
    return runs[0]


def same_bits(got, want, what):
    bits = torch.int16 if got.dtype == BF16 else torch.int32
    bad = got.contiguous().view(bits) != want.contiguous().view(bits)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}: " \
                                f"{got[bad][0].item()} != {want[bad][0].item()}"


@pytest.mark.parametrize("case", list(K.CASES))
def test_q8_dwconv2d_is_exact(nv, case):
    """Bit equality with the exact sums pushed through the stated rounding chain: bare sums, then bias with a per-tensor and a
    per-channel factor, bf16 and fp32 outputs, the fp32 identity fold on and off."""
    ops = K.operands(case)
    exact, bias, scale = ops["exact"], ops["bias"], ops["scale"]
    if case == "m128":
        assert float(exact.max()) == float(exact.min()) == 49 * 16384
    if case == "pm127":
        assert float(exact.abs().max()) == 9 * 16129          # the interior: every product of the window has the same sign
        assert float(exact.max()) == -float(exact.min())      # and both signs occur
    same_bits(q8_dwconv(nv, case, ops, F32, None, None, 0, 0), K.chain(exact, None, None, F32, 0), f"{case} bare fp32")
    same_bits(q8_dwconv(nv, case, ops, BF16, None, None, 0, 0), K.chain(exact, None, None, BF16, 0), f"{case} bare bf16")
    for per_col in (0, 1):
        s = scale if per_col else scale[:1].clone()
        for fold in (0, 1):
            same_bits(q8_dwconv(nv, case, ops, F32, bias, s, per_col, fold), K.chain(exact, bias, s, F32, fold), f"{case} fp32 {per_col} {fold}")
        b16, s16 = bias.bfloat16(), s.bfloat16()
        same_bits(q8_dwconv(nv, case, ops, BF16, b16, s16, per_col, 0), K.chain(exact, b16, s16, BF16, 0), f"{case} bf16 {per_col}")


def test_q8_dwconv2d_declines_on_the_device(nv):
    """A misaligned pointer, C = 24, kh kw = 1024: refused before any launch; the output buffer keeps its sentinel."""
    x = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    w = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    y = torch.full((4096,), float("nan"), dtype=F32, device="cuda")
    s = torch.ones(64, dtype=F32, device="cuda")

    def call(xp=x.data_ptr(), wp=w.data_ptr(), yp=y.data_ptr(), bias=None, sp=None, c=16, h=4, wd=4, kh=1, kw=1, n=1):
        return nv.lib().qt_q8_dwconv2d(xp, wp, yp, 1, bias, sp, 0, 0, n, h, wd, c, kh, kw, 1, 1, 0, 0, 1, 1, stream())
    assert call(c=24) == nv.QT_ERR_BAD_ARG
    assert call(kh=32, kw=32, h=32, wd=32) == nv.QT_ERR_BAD_ARG
    assert call(xp=x.data_ptr() + 1) == nv.QT_ERR_UNALIGNED and call(wp=w.data_ptr() + 8) == nv.QT_ERR_UNALIGNED
    assert call(yp=y.data_ptr() + 4) == nv.QT_ERR_UNALIGNED and call(sp=s.data_ptr() + 4) == nv.QT_ERR_UNALIGNED
    assert call(bias=s.data_ptr() + 8) == nv.QT_ERR_UNALIGNED
    assert call(n=0) == 0 and call(h=2, wd=2, kh=3, kw=3) == 0
    torch.cuda.synchronize()
    assert bool(y.isnan().all())


# ---- the operator ---------------------------------------------------------------------------------------------------------------
def int8_map(device):
    import quantized_training as qt
    return qt.get_quantization_map("int8", torch.device(device))


def op_args(dtype, n=2, cin=48, h=9, w=7, cout=None, k=(3, 3), per_channel=False, seed=0, groups=None, wcin=1):
    cout = cin if cout is None else cout
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, cin, h, w, generator=g) * 2).to(dtype).cuda()
    scale = torch.tensor(0.04).to(dtype).cuda()
    wc = torch.randint(-127, 128, (cout, *k, wcin), generator=g).to(torch.int8).cuda()
    b = torch.randint(-4000, 4000, (cout,), generator=g).to(dtype).cuda()
    out_scale = (torch.rand(cout, 1, 1, generator=g) * 1e-3 + 1e-4 if per_channel else torch.tensor([3e-4])).to(dtype).cuda()
    return x, scale, int8_map("cuda"), wc, b, out_scale, (cin if groups is None else groups)


def unfused(x, scale, qmap, wc, b, stride, padding, dilation, groups, out_scale, out_map):
    """The three nodes of the parent graph on the tensors it stored: the weight as [Cout, Cin / groups, kh, kw] values."""
    xq = torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap)
    y = F.conv2d(xq, wc.permute(0, 3, 1, 2).to(x.dtype).contiguous(), b, stride, padding, dilation, groups)
    return torch.ops.quantized_ops.dequantize(y, out_scale, None, None, None, out_map)


def rows_of(t):
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).cpu()


def conv_exact(xq, wv, stride, padding, dilation, groups):
    y = F.conv2d(xq.double(), wv.double(), None, stride, padding, dilation, groups)
    return y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, y.shape[1]).contiguous()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_depthwise_operator_equals_the_exact_reference(nv, monkeypatch, dtype, per_channel, layout):
    """conv2d_q with groups = C on the device: the native route (STATS["conv2d_dw_int8"] moves, conv2d_int8 does not), bit for bit the
    exact chain built from its own arguments and bit for bit the three nodes run on the host; against the three nodes run on the
    device every element within layer_bound with K = kh kw (a library kernel may round before the bias add)."""
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    x, scale, qmap, wc, b, out_scale, groups = op_args(dtype, per_channel=per_channel)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    stride, padding, dilation = [2, 1], [1, 2], [1, 2]
    ident = int8_map("cuda").new_empty(0)           # any tensor: the identity map's content is not read by the native route
    before = dict(pt2e_native.STATS)
    xq = torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap).cpu()
    wv = wc.cpu().permute(0, 3, 1, 2)
    exact = conv_exact(xq, wv, stride, padding, dilation, groups)
    for out_map in (None, ident):
        y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, wc, b, stride, padding, dilation, groups, out_scale, out_map, "int8")
        assert y.shape == (2, 48, 5, 7) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
        want = K.chain(exact, b.cpu(), out_scale.cpu().reshape(-1), dtype, int(out_map is not None))
        same_bits(rows_of(y), want, f"conv2d_q depthwise {dtype} {layout}")
    assert pt2e_native.STATS["conv2d_dw_int8"] - before["conv2d_dw_int8"] == 2 and pt2e_native.STATS["conv2d_int8"] == before["conv2d_int8"]
    y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, wc, b, stride, padding, dilation, groups, out_scale, None, "int8")
    host = unfused(x.cpu(), scale.cpu(), qmap.cpu(), wc.cpu(), b.cpu(), stride, padding, dilation, groups, out_scale.cpu(), None)
    same_bits(rows_of(y), rows_of(host), "conv2d_q depthwise against the three nodes on the host")
    dev = unfused(x, scale, qmap, wc, b, stride, padding, dilation, groups, out_scale, None)
    _, bound = K.layer_bound(exact, conv_exact(xq.abs(), wv.abs(), stride, padding, dilation, groups), 9, b, out_scale, dtype)
    diff = (rows_of(y).double() - rows_of(dev).double()).abs()
    bits = torch.int16 if dtype == BF16 else torch.int32
    share = float((rows_of(y).contiguous().view(bits) == rows_of(dev).contiguous().view(bits)).float().mean())
    print(f"depthwise {dtype} {layout}: bit-equal to the device's three nodes on {share:.4f} of the elements; worst |diff| / bound = "
          f"{float((diff / bound).max()):.3f}")
    assert bool((diff <= bound).all())


FALLBACKS = {
    "groups_2": dict(cin=32, groups=2, wcin=16),
    "depth_multiplier": dict(cin=16, cout=32, groups=16),
    "c_24": dict(cin=24),
    "fp16": dict(dtype=torch.float16),
    "misaligned": dict(offset=1),
    "dw_rule": dict(rule="_conv_q_dw_route_takes"),
    "pw_rule": dict(rule="_conv_q_pw16_route_takes", cin=16, cout=96, groups=1, wcin=16, k=(1, 1), padding=[0, 0]),
    "strided_1x1_over_16": dict(cin=16, cout=96, groups=1, wcin=16, k=(1, 1), padding=[0, 0], stride=[2, 2]),
}


@pytest.mark.parametrize("which", list(FALLBACKS))
def test_operator_fallbacks_equal_the_unfused_graph(nv, monkeypatch, which):
    """Everything the kernels do not take runs quantize -> aten.conv2d -> dequantize verbatim: the same bits as those three nodes on
    the same device, no native launch counted, and the reason recorded."""
    from quantized_training import pt2e_native
    cfg = dict(FALLBACKS[which])
    rule = cfg.pop("rule", None)
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", rule is not None)
    for name in ("_conv_q_dw_route_takes", "_conv_q_pw16_route_takes"):
        monkeypatch.setattr(pt2e_native, name, lambda *a, _n=name: _n != rule)
    dtype, offset = cfg.pop("dtype", BF16), cfg.pop("offset", 0)
    stride, padding = cfg.pop("stride", [1, 1]), cfg.pop("padding", [1, 1])
    x, scale, qmap, wc, b, out_scale, groups = op_args(dtype, **cfg)
    if offset:
        base = torch.zeros(x.numel() + 8, dtype=dtype, device="cuda")
        base[offset:offset + x.numel()] = x.reshape(-1)
        x = base[offset:offset + x.numel()].view(x.shape)
        assert x.data_ptr() % 16 != 0
    before, reasons = dict(pt2e_native.STATS), sum(pt2e_native.CONV_Q_REASONS.values())
    y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, wc, b, stride, padding, [1, 1], groups, out_scale, None, "int8")
    want = unfused(x, scale, qmap, wc, b, stride, padding, [1, 1], groups, out_scale, None)
    assert dict(pt2e_native.STATS) == before and sum(pt2e_native.CONV_Q_REASONS.values()) == reasons + 1
    assert y.dtype == want.dtype and y.shape == want.shape
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("cin,cout", [(16, 96), (144, 32)])
def test_pointwise_route_equals_the_exact_reference(nv, monkeypatch, dtype, cin, cout):
    """A 1 x 1, stride 1, unpadded call over Cin = 16 mod 32: codes pass + qt_q8_gemm, counted in conv2d_int8, bit for bit the exact
    chain, from NCHW and channels_last input, with a per-tensor and a per-channel factor."""
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    for per_channel, layout in ((False, "nchw"), (True, "channels_last")):
        x, scale, qmap, wc, b, out_scale, _ = op_args(dtype, cin=cin, cout=cout, h=6, w=6, k=(1, 1), wcin=cin, per_channel=per_channel, groups=1)
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
        before = dict(pt2e_native.STATS)
        y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, wc, b, [1, 1], [0, 0], [1, 1], 1, out_scale, None, "int8")
        assert pt2e_native.STATS["conv2d_int8"] - before["conv2d_int8"] == 1 and pt2e_native.STATS["conv2d_dw_int8"] == before["conv2d_dw_int8"]
        assert y.shape == (2, cout, 6, 6) and y.is_contiguous(memory_format=torch.channels_last)
        xq = torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap).cpu()
        exact = conv_exact(xq, wc.cpu().permute(0, 3, 1, 2), 1, 0, 1, 1)
        same_bits(rows_of(y), K.chain(exact, b.cpu(), out_scale.cpu().reshape(-1), dtype, 0), f"pointwise {cin} -> {cout} {dtype} {layout}")


# ---- the converted block ----------------------------------------------------------------------------------------------------------
def converted(native, monkeypatch):
    monkeypatch.setenv("QT_PT2E_NATIVE", native)
    return K.convert_block(BF16, device="cuda", native=None)


def targets(gm):
    return [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]


def test_converted_block_runs_conv2d_q(nv, monkeypatch):
    """Device conversion with QT_PT2E_NATIVE=1: expand, depthwise and project are conv2d_q nodes, the stem stays aten.conv2d; with =0
    the graph is upstream's.  Layer by layer, on the native graph's own layer inputs, |native node - three nodes| <= the derived bound
    per element, for the three nodes run on the device and on the host."""
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    g0, x = converted("0", monkeypatch)
    g1, _ = converted("1", monkeypatch)
    t0, t1 = targets(g0), targets(g1)
    assert t0.count("aten.conv2d.default") == 4 and not any("conv2d_q" in t for t in t0)
    assert t1.count("aten.conv2d.default") == 1 and t1.count("quantized_ops.conv2d_q.default") == 3
    assert tuple(g1.dw_weight_codes.shape) == (96, 3, 3, 1) and tuple(g1.expand_weight_codes.shape) == (96, 1, 1, 16)
    assert tuple(g1.project_weight_codes.shape) == (32, 1, 1, 96)
    before = dict(pt2e_native.STATS)
    with torch.no_grad():
        y0 = g0(x)
    assert dict(pt2e_native.STATS) == before
    with torch.no_grad():
        y1 = g1(x)
    ran = {k: pt2e_native.STATS[k] - before[k] for k in before}
    assert ran["conv2d_dw_int8"] == 1 and ran["conv2d_int8"] == 2, ran
    assert y1.shape == y0.shape and bool(y1.float().isfinite().all())

    checked = []

    class PerLayer(torch.fx.Interpreter):
        def call_function(self, target, args, kwargs):
            out = super().call_function(target, args, kwargs)
            if target == torch.ops.quantized_ops.conv2d_q.default:
                inp, scale, qmap, wc, b, stride, padding, dilation, groups, out_scale, out_map, _ = args
                xq = torch.ops.quantized_ops.quantize(inp, scale, None, None, None, qmap).cpu()
                wv = wc.cpu().permute(0, 3, 1, 2)
                k = wc.shape[1] * wc.shape[2] * wc.shape[3]
                exact = conv_exact(xq, wv, stride, padding, dilation, groups)
                _, bound = K.layer_bound(exact, conv_exact(xq.abs(), wv.abs(), stride, padding, dilation, groups), k, b, out_scale, inp.dtype)
                dev = unfused(inp, scale, qmap, wc, b, stride, padding, dilation, groups, out_scale, out_map)
                host = unfused(inp.cpu(), scale.cpu(), qmap.cpu(), wc.cpu(), b.cpu(), stride, padding, dilation, groups, out_scale.cpu(),
                               out_map.cpu() if out_map is not None else None)
                for other, what in ((dev, "device graph"), (host, "host graph")):
                    diff = (rows_of(out).double() - rows_of(other).double()).abs()
                    print(f"conv2d_q {tuple(wc.shape)}: worst |native - {what}| / bound = {float((diff / bound).max()):.3f}")
                    assert bool((diff <= bound).all()), f"native vs the {what}, layer {tuple(wc.shape)}"
                checked.append(tuple(wc.shape))
            return out

    with torch.no_grad():
        PerLayer(g1).run(x)
    assert checked == [(96, 1, 1, 16), (96, 3, 3, 1), (32, 1, 1, 96)]


def test_converted_block_graph_capture(nv, monkeypatch):
    """A torch.cuda.graph replay of the converted block equals the eager call bit for bit; the capture takes no fallback (three native
    launches, no new reason) and reads nothing on the host (a host read would fail the capture)."""
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
    before, reasons = dict(pt2e_native.STATS), sum(pt2e_native.CONV_Q_REASONS.values())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = g1(static_x)
    assert pt2e_native.STATS["conv2d_dw_int8"] - before["conv2d_dw_int8"] == 1 and pt2e_native.STATS["conv2d_int8"] - before["conv2d_int8"] == 2
    assert sum(pt2e_native.CONV_Q_REASONS.values()) == reasons
    static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), e1.view(torch.int16))
