"""conv2d_mx on the device: qt_conv2d_mx (csrc/qt_mx_conv.hip) through the C ABI, the three sources of its activation operand, the
operator, its fallbacks and a converted CNN.

Exact tier: element values out of {0, +-0.5, +-1, +-2} (in all five formats) and block scales out of {0.5, 1, 2}: every product is a
multiple of 2^-4 of magnitude <= 16 and every partial sum is exact in fp32, so the fp32 result must equal the fp64 convolution of the
dequantized operands bit for bit, and the bf16 result that value (+ a bias of small integers) rounded once.
Tolerance tier: operands from quantize_mx of randn; |err| <= 2^-14 conv(|x|, |w|) (+ 2^-8 |want| for bf16) against fp64, the bound of
test_mx_gemm_vs_dequantized_reference.
The codes and E8M0 bytes sit between margins of 0xFF (NaN in e4m3, so a read outside the image shows in the result), the output
between margins of NaN."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_launch import nv, stream  # noqa: F401
from oracle import qt_oracle as o

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
FMT_ID = {"fp8_e4m3": 0, "fp8_e5m2": 1, "fp6_e2m3": 2, "fp6_e3m2": 3, "fp4_e2m1": 4}
BITS = {"fp8_e4m3": 8, "fp8_e5m2": 8, "fp6_e2m3": 6, "fp6_e3m2": 6, "fp4_e2m1": 4}
PAIRS = [("fp8_e4m3", "fp8_e4m3"), ("fp8_e4m3", "fp8_e5m2"), ("fp8_e5m2", "fp8_e4m3"), ("fp8_e5m2", "fp8_e5m2"), ("fp6_e2m3", "fp6_e2m3"),
         ("fp6_e3m2", "fp6_e3m2"), ("fp4_e2m1", "fp4_e2m1"), ("fp8_e4m3", "fp4_e2m1"), ("fp6_e2m3", "fp4_e2m1"), ("fp6_e3m2", "fp4_e2m1")]

# (N, H, W, Cin, Cout, (kh, kw), stride, padding, dilation)
CASES = {
    "A": (1, 5, 5, 32, 16, (3, 3), (1, 1), (1, 1), (1, 1)),      # K = 288: a ragged K tail; one ragged M tile, ragged N
    "B": (2, 9, 7, 64, 136, (3, 3), (2, 2), (1, 1), (1, 1)),     # stride, two N tiles
    "C": (1, 12, 12, 128, 64, (1, 1), (1, 1), (0, 0), (1, 1)),   # one K step, two M tiles
    "D": (3, 8, 6, 32, 32, (3, 2), (1, 2), (2, 0), (2, 1)),      # asymmetric in every parameter
    "E": (1, 4, 4, 256, 8, (4, 4), (1, 1), (0, 0), (1, 1)),      # one output pixel, 32 K steps
    "F": (2, 7, 7, 96, 40, (3, 3), (1, 1), (1, 1), (1, 1)),      # K tiles straddle taps; H W % 8 != 0
    "G": (1, 3, 3, 32, 16, (1, 1), (1, 1), (1, 1), (1, 1)),      # border outputs are the bias alone
}
WIDE = [k for k, c in CASES.items() if c[3] % 64 == 0]            # what the 6-bit formats take


def out_hw(case):
    n, h, w, cin, cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw) = CASES[case]
    return (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def conv64(case, x, w):
    """fp64 convolution on the host -> NHWC [N, Ho, Wo, Cout]"""
    _, _, _, _, _, _, stride, padding, dilation = CASES[case]
    return F.conv2d(x.double(), w.double(), None, stride, padding, dilation).permute(0, 2, 3, 1).contiguous()


def nhwc_rows(t):
    """[A, C, H, W] -> [A H W, C] (numpy, fp64)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().numpy()


@functools.lru_cache(maxsize=None)
def exact_operands(case, fx, fw):
    """Host operands of the exact tier: packed codes / E8M0 bytes of x (NHWC) and w ([Cout][kh kw Cin]), and the fp64 result."""
    n, h, w, cin, cout, (kh, kw), _, _, _ = CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case + fx + fw)))
    values, scales = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0]), torch.tensor([0.5, 1.0, 2.0])
    xv = values[torch.randint(0, 7, (n, cin, h, w), generator=g)]
    wv = values[torch.randint(0, 7, (cout, cin, kh, kw), generator=g)]
    xs = scales[torch.randint(0, 3, (n, cin // 32, h, w), generator=g)]
    ws = scales[torch.randint(0, 3, (cout, cin // 32, kh, kw), generator=g)]
    x_codes, x_e8 = o.mx_pack(nhwc_rows(xv), nhwc_rows(xs), fx, 32)
    w_codes, w_e8 = o.mx_pack(nhwc_rows(wv).reshape(cout, -1), nhwc_rows(ws).reshape(cout, -1), fw, 32)
    ref = conv64(case, xv.double() * xs.double().repeat_interleave(32, 1), wv.double() * ws.double().repeat_interleave(32, 1))
    return dict(xv=xv, xs=xs, wv=wv, ws=ws, x_codes=x_codes, x_e8=x_e8, w_codes=w_codes, w_e8=w_e8, ref=ref)


class Margins:
    """A byte array on the device between two margins of `fill`."""
    PAD = 256

    def __init__(self, host, fill=0xFF):
        host = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        self.n = host.size
        self.raw = torch.full((self.n + 2 * self.PAD,), fill, dtype=torch.uint8, device="cuda")
        self.raw[self.PAD:self.PAD + self.n] = torch.from_numpy(host).cuda()
        assert (self.raw.data_ptr() + self.PAD) % 16 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.PAD


def run_c(nv, case, ops, fx, fw, dtype, bias):
    """qt_conv2d_mx twice into NaN-filled buffers: status 0, the margins still NaN, both runs the same bits -> y [N, Ho, Wo, Cout] (host)."""
    n, h, w, cin, cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw) = CASES[case]
    ho, wo = out_hw(case)
    count, pad = n * ho * wo * cout, 64
    xc, xe, wc, we = Margins(ops["x_codes"]), Margins(ops["x_e8"]), Margins(ops["w_codes"]), Margins(ops["w_e8"])
    b = bias.to(dtype).cuda() if bias is not None else None
    runs = []
    for _ in range(2):
        buf = torch.full((count + 2 * pad,), float("nan"), dtype=dtype, device="cuda")
        rc = nv.lib().qt_conv2d_mx(xc.ptr, xe.ptr, FMT_ID[fx], wc.ptr, we.ptr, FMT_ID[fw], buf.data_ptr() + pad * buf.element_size(),
                                   int(dtype == F32), b.data_ptr() if b is not None else None, n, h, w, cin, cout, kh, kw, sh, sw, ph, pw,
                                   dh, dw, stream())
        assert rc == 0, f"case {case} {fx} x {fw}: status {rc}"
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool(host[:pad].isnan().all()) and bool(host[pad + count:].isnan().all()), f"case {case}: a margin of y was written"
        runs.append(host[pad:pad + count].reshape(n, ho, wo, cout))
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(runs[0].view(bits), runs[1].view(bits)), f"case {case}: two launches differ"
    return runs[0]


def assert_exact(nv, case, fx, fw):
    ops = exact_operands(case, fx, fw)
    cout = CASES[case][4]
    ref = ops["ref"]
    assert torch.equal(ref.float().double(), ref)                                          # the reference itself is an fp32 number
    y = run_c(nv, case, ops, fx, fw, F32, None)
    bad = (y.double() != ref)
    assert not bool(bad.any()), f"case {case} {fx} x {fw}, fp32: {int(bad.sum())} of {bad.numel()} differ, largest {float((y.double() - ref).abs().max())}"
    bias = torch.arange(cout, dtype=torch.float64) % 7 - 3                                 # small integers
    for dtype in (BF16, F32):
        y = run_c(nv, case, ops, fx, fw, dtype, bias)
        want = (ref + bias).float().to(dtype)                                             # (exact in fp32) rounded once
        bad = y.double() != want.double()
        assert not bool(bad.any()), f"case {case} {fx} x {fw}, {dtype} with bias: {int(bad.sum())} of {bad.numel()} differ"
    if case == "G":                                                                        # the border sees padding only
        assert torch.equal(y[0, 0, 0].double(), bias) and torch.equal(y[0, -1, -1].double(), bias)


# ---- 1. exact tier ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp8_e4m3", "fp4_e2m1"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_whole_grid(nv, case, fmt):
    assert_exact(nv, case, fmt, fmt)


@pytest.mark.parametrize("case", WIDE)
def test_exact_six_bit_grid(nv, case):
    assert WIDE == ["B", "C", "E"]
    assert_exact(nv, case, "fp6_e2m3", "fp6_e2m3")


@pytest.mark.parametrize("fx,fw", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_exact_every_pair(nv, fx, fw):
    from quantized_training import mx_gemm
    assert {(FMT_ID[a], FMT_ID[b]) for a, b in PAIRS} == mx_gemm._PAIRS
    assert_exact(nv, "B" if 6 in (BITS[fx], BITS[fw]) else "A", fx, fw)
    assert_exact(nv, "C", fx, fw)


def device_operands(case, fmt, dtype, layout="nchw"):
    """The exact tier's values and scales as device tensors that carry what quantize_mx would have left on them."""
    ops = exact_operands(case, fmt, fmt)
    x, xs, w, ws = (ops[k].to(dtype).cuda() for k in ("xv", "xs", "wv", "ws"))
    if layout == "nhwc":
        x, xs = x.contiguous(memory_format=torch.channels_last), xs.contiguous(memory_format=torch.channels_last)
    from quantized_training import mx_operand
    for t in (x, w):
        mx_operand.set_format(t, fmt)
    for s in (xs, ws):
        mx_operand.set_pow2(s)
    return ops, x, xs, w, ws


def test_exact_block_size_64(nv):
    """Blocks of 64 channels: the packer repeats each scale byte; case C (Cin = 128) with scales that are constant over 64 channels."""
    from quantized_training import mx_gemm, mx_operand
    n, h, w, cin, cout, (kh, kw), stride, padding, dilation = CASES["C"]
    ops, x, xs, wt, ws = device_operands("C", "fp8_e4m3", F32)
    xs64, ws64 = mx_operand.set_pow2(xs[:, ::2].contiguous()), mx_operand.set_pow2(ws[:, ::2].contiguous())
    ref = conv64("C", ops["xv"].double() * ops["xs"][:, ::2].double().repeat_interleave(64, 1),
                 ops["wv"].double() * ops["ws"][:, ::2].double().repeat_interleave(64, 1))
    mx_gemm.STATS.reset()
    y = torch.ops.quantized_ops.conv2d_mx(x, wt, None, stride, padding, dilation, 1, input_scale=xs64, weight_scale=ws64, block_size=64)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0)
    assert y.shape == (n, cout, 12, 12) and y.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(y.permute(0, 2, 3, 1).cpu().double(), ref)


# ---- 2. tolerance tier -----------------------------------------------------------------------------------------------------------------
def qmax_of(name):
    from quantized_training.quantizer.quantizer import get_quant_min_max
    return float(get_quant_min_max(name)[1])


def quantized(t, fmt, bs=32):
    from quantized_training.fake_quantize import get_quantization_map
    return torch.ops.quantized_ops.quantize_mx(t, get_quantization_map(fmt, "cuda"), [1], bs, qmax_of(fmt), True, None, None)


def dequantized64(q, s, bs=32):
    return q.cpu().double() * s.cpu().double().repeat_interleave(bs, 1)


def within_bound(y, want, mag, dtype, what):
    err = (y.permute(0, 2, 3, 1).cpu().double() - want).abs()
    tol = 2.0 ** -14 * mag + (2.0 ** -8 * want.abs() if dtype == BF16 else 0.0)
    assert bool((err <= tol).all()), f"{what}: largest error {float(err.max())}, {int((err > tol).sum())} of {err.numel()} outside the bound"


@pytest.mark.parametrize("fmt", ["fp8_e4m3", "fp4_e2m1"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_tolerance_whole_grid(nv, case, fmt):
    from quantized_training import mx_gemm, mx_operand
    n, h, w, cin, cout, (kh, kw), stride, padding, dilation = CASES[case]
    g = torch.Generator().manual_seed(7)
    x0, w0, b0 = torch.randn(n, cin, h, w, generator=g) * 2, torch.randn(cout, cin, kh, kw, generator=g) * 0.5, torch.randn(cout, generator=g)
    for dtype in (BF16, F32):
        xs, xq = quantized(x0.to(dtype).cuda().contiguous(memory_format=torch.channels_last), fmt)     # what a layer inside a network receives
        ws, wq = quantized(w0.to(dtype).cuda(), fmt)
        assert mx_operand.operand_record(xq, mx_operand.NHWC) is not None
        dx, dw_ = dequantized64(xq, xs), dequantized64(wq, ws)
        ref, mag = conv64(case, dx, dw_), conv64(case, dx.abs(), dw_.abs())
        for bias in (None, b0.to(dtype).cuda()):
            mx_gemm.STATS.reset()
            y = torch.ops.quantized_ops.conv2d_mx(xq, wq, bias, stride, padding, dilation, 1, input_scale=xs, weight_scale=ws, block_size=32)
            assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0)
            assert y.dtype == dtype and y.shape == (n, cout) + out_hw(case)
            want = ref + (bias.cpu().double() if bias is not None else 0.0)
            within_bound(y, want, mag, dtype, f"case {case} {fmt} {dtype} bias={bias is not None}")


# ---- 3. graph capture ------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager(nv):
    case, fmt = "B", "fp8_e4m3"
    n, h, w, cin, cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw) = CASES[case]
    ops = exact_operands(case, fmt, fmt)
    ho, wo = out_hw(case)
    dev = {k: torch.from_numpy(ops[k]).cuda() for k in ("x_codes", "x_e8", "w_codes", "w_e8")}
    bias = (torch.arange(cout) % 5).to(BF16).cuda()

    def run(y):
        assert nv.lib().qt_conv2d_mx(dev["x_codes"].data_ptr(), dev["x_e8"].data_ptr(), 0, dev["w_codes"].data_ptr(), dev["w_e8"].data_ptr(), 0,
                                     y.data_ptr(), 0, bias.data_ptr(), n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, stream()) == 0

    eager = torch.zeros(n, ho, wo, cout, dtype=BF16, device="cuda")
    run(eager)
    torch.cuda.synchronize()
    captured = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                    # one stream, no parallel branches
            run(captured)
    torch.cuda.current_stream().wait_stream(side)
    captured.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.view(torch.int16), eager.view(torch.int16))
    assert torch.equal(eager.cpu().double(), (ops["ref"] + bias.cpu().double()).float().to(BF16).double())


# ---- 4. the three sources of the activation operand ----------------------------------------------------------------------------------------
def bits_of(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.parametrize("case", ["B", "F", "C"])
def test_activation_operand_sources_agree(nv, case):
    """quantize_mx of an NCHW-contiguous tensor (the strided pass: takes the pack only where H W is a multiple of 8), of a
    channels_last one (the last-axis pass on the stored tensor) and qt_mx_pack through the strides of either layout: the same codes
    and E8M0 bytes as the host packer makes of the CPU composite's values and scales, and the same conv2d_mx bits."""
    from quantized_training import mx_conv, mx_gemm, mx_operand
    from quantized_training.fake_quantize import get_quantization_map, mx_block_view
    fmt = "fp8_e4m3"
    n, h, w, cin, cout, (kh, kw), stride, padding, dilation = CASES[case]
    g = torch.Generator().manual_seed(11)
    x0, w0 = (torch.randn(n, cin, h, w, generator=g) * 2).to(BF16), (torch.randn(cout, cin, kh, kw, generator=g) * 0.5).to(BF16)
    host_map = get_quantization_map(fmt, "cpu")
    s_ref = torch.ops.quantized_ops.calculate_mx_qparam(x0, [1], 32, 448.0, True, None)
    q_ref = torch.ops.quantized_ops.quantize(x0, s_ref, None, [1], 32, host_map)
    want_codes, want_e8 = o.mx_pack(nhwc_rows(q_ref), nhwc_rows(s_ref), fmt, 32)

    s1, q1 = quantized(x0.cuda(), fmt)                                                     # NCHW-contiguous
    s2, q2 = quantized(x0.cuda().contiguous(memory_format=torch.channels_last), fmt)       # channels_last-dense
    for s, q in ((s1, q1), (s2, q2)):
        assert torch.equal(bits_of(q), bits_of(q_ref)) and torch.equal(bits_of(s), bits_of(s_ref))
        assert mx_operand.format_of(q) == fmt and mx_operand.is_pow2(s)
    assert q1.is_contiguous() and q2.permute(0, 2, 3, 1).is_contiguous() and s2.permute(0, 2, 3, 1).is_contiguous()
    taken = mx_block_view(tuple(x0.shape), BF16, 32, [1]) is not None
    assert taken == ((h * w) % 8 == 0) == (case == "C")
    assert (mx_operand.operand_record(q1, mx_operand.NHWC) is not None) == taken             # declined by the kernel: nothing is set
    assert mx_operand.operand_record(q2, mx_operand.NHWC) is not None and mx_operand.operand_record(q2, mx_operand.ROWS) is None

    ws, wq = quantized(w0.cuda(), fmt)
    results = {}
    for name, s, q, strip in (("nchw as left by quantize_mx", s1, q1, False), ("channels_last producer", s2, q2, False),
                              ("nchw through qt_mx_pack", s1, q1, True), ("channels_last through qt_mx_pack", s2, q2, True)):
        if strip:
            mx_operand.drop_operand(q)
        codes, e8 = mx_conv._activation_operand(q, s, 0, 32)
        pre = mx_operand.operand_record(q, mx_operand.NHWC)
        assert (pre is not None and codes is pre[2]) == (not strip and (taken or q is q2)), name
        assert np.array_equal(codes.cpu().numpy(), want_codes), f"{name}: codes"
        assert np.array_equal(e8.cpu().numpy(), want_e8), f"{name}: E8M0 bytes"
        mx_gemm.STATS.reset()
        results[name] = torch.ops.quantized_ops.conv2d_mx(q, wq, None, stride, padding, dilation, 1, input_scale=s, weight_scale=ws, block_size=32)
        assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0), name
    first = results.pop("nchw as left by quantize_mx")
    for name, y in results.items():
        assert torch.equal(bits_of(y), bits_of(first)), name


# ---- 5. the operator and its fallbacks -------------------------------------------------------------------------------------------------
def composite_operands(x, w, xs, ws, bs, x_code=None, w_code=None):
    """decomposed.py:289-300 restated: codebook lookup, then the block scales repeated along the channel axis"""
    if x_code is not None:
        x = x_code[x.to(torch.long)].to(x.dtype)
    if w_code is not None:
        w = w_code[w.to(torch.long)].to(w.dtype)
    return x * xs.repeat_interleave(bs, 1), w * ws.repeat_interleave(bs, 1)


def test_operator_goes_native_and_every_reachable_reason_falls_back(nv, monkeypatch):
    from quantized_training import mx_gemm, mx_operand
    case = "B"
    n, h, w, cin, cout, (kh, kw), stride, padding, dilation = CASES[case]
    g = torch.Generator().manual_seed(13)
    x0, w0 = (torch.randn(n, cin, h, w, generator=g) * 2).to(BF16).cuda(), (torch.randn(cout, cin, kh, kw, generator=g) * 0.5).to(BF16).cuda()
    bias = torch.randn(cout, generator=g).to(BF16).cuda()
    conv = torch.ops.quantized_ops.conv2d_mx

    def fresh(fx="fp8_e4m3", fw="fp8_e4m3", bs=32, wsrc=w0, xsrc=x0):
        (xs, xq), (ws, wq) = quantized(xsrc, fx, bs), quantized(wsrc, fw, bs)
        return dict(x=xq, w=wq, xs=xs, ws=ws, bs=bs, groups=1, x_code=None, w_code=None)

    def check(p, native, what, cast=lambda t: t):
        """A native call meets the tolerance tier's bound against fp64; a call that falls back IS the composite: the same ops on the same
        tensors, compared bit for bit with their restatement."""
        p = {k: (cast(v) if isinstance(v, torch.Tensor) else v) for k, v in p.items()}
        b = cast(bias)
        mx_gemm.STATS.reset()
        y = conv(p["x"], p["w"], b, stride, padding, dilation, p["groups"], input_scale=p["xs"], weight_scale=p["ws"], block_size=p["bs"],
                 input_code=p["x_code"], weight_code=p["w_code"])
        assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == native, what
        if native == (1, 0):
            dx, dw_ = dequantized64(p["x"], p["xs"], p["bs"]), dequantized64(p["w"], p["ws"], p["bs"])
            within_bound(y, conv64(case, dx, dw_) + b.cpu().double(), conv64(case, dx.abs(), dw_.abs()), BF16, what)
            return
        dx, dw_ = composite_operands(p["x"], p["w"], p["xs"], p["ws"], p["bs"], p["x_code"], p["w_code"])
        want = F.conv2d(dx, dw_, b, stride, padding, dilation, p["groups"])
        assert y.shape == want.shape and y.dtype == want.dtype and torch.equal(y.view(torch.int16), want.view(torch.int16)), what

    check(fresh(), (1, 0), "device operands from quantize_mx")
    p = fresh(); p["groups"] = 2; p["w"], p["ws"] = p["w"][:, :32].contiguous(), p["ws"][:, :1].contiguous()
    mx_operand.set_format(p["w"], "fp8_e4m3"), mx_operand.set_pow2(p["ws"])
    check(p, (0, 1), "groups = 2")
    p = fresh()
    p["x"] = torch.randint(0, 16, p["x"].shape, device="cuda").to(BF16); p["x_code"] = torch.linspace(-4, 4, 16, device="cuda").to(BF16)
    check(p, (0, 0), "an input codebook")
    check(fresh(bs=16), (0, 0), "block size 16")
    p = fresh(); p["x"] = p["x"].clone()
    check(p, (0, 1), "an input without a remembered format")
    p = fresh(); p["xs"] = p["xs"].clone()
    check(p, (0, 1), "an input scale not flagged power-of-two")
    p = fresh(); p["ws"] = p["ws"].clone()
    check(p, (0, 1), "a weight scale not flagged power-of-two")
    p = fresh(); p["w"] = (p["w"] * 0 + 0.3).to(BF16); p["ws"] = mx_operand.set_pow2(p["ws"].clone())
    check(p, (0, 1), "a weight the packer refuses in every format")
    check(fresh(fx="fp4_e2m1", fw="fp8_e4m3"), (0, 1), "fp4 x fp8: a pair without a kernel")
    check(fresh(), (0, 0), "fp16", cast=lambda t: t.half())
    # profiles/conv2d_mx.txt: a 1 x 1 filter over 64 channels (half a k tile) goes native on the operand quantize_mx left (channels_last input) and
    # stays with the composite where qt_mx_pack would have to run first (9 x 7 planes: the strided pass leaves nothing)
    w1 = (torch.randn(cout, cin, 1, 1, generator=g) * 0.5).to(BF16).cuda()
    p = fresh(wsrc=w1)
    assert mx_operand.operand_record(p["x"], mx_operand.NHWC) is None
    check(p, (0, 1), "1 x 1, 64 -> 136 without a packed operand")
    p = fresh(wsrc=w1, xsrc=x0.contiguous(memory_format=torch.channels_last))
    assert mx_operand.operand_record(p["x"], mx_operand.NHWC) is not None
    check(p, (1, 0), "1 x 1, 64 -> 136 on the operand quantize_mx left")
    monkeypatch.setenv("QT_MX_GEMM", "0")
    check(fresh(), (0, 0), "QT_MX_GEMM=0")


# ---- 6. a converted CNN ----------------------------------------------------------------------------------------------------------------
class ToyCNN(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.c1 = torch.nn.Conv2d(3, 32, 3)
        self.c2 = torch.nn.Conv2d(32, 64, 3, stride=2, padding=1)
        self.c3 = torch.nn.Conv2d(64, 64, 1)

    def forward(self, x):
        return self.c3(torch.relu(self.c2(torch.relu(self.c1(x)))))


def test_converted_cnn_runs_its_eligible_layers_natively(nv):
    from quantized_training import mx_gemm, mx_operand, quantize_pt2e as qp
    torch.manual_seed(0)
    m = ToyCNN().eval().to(BF16).cuda()
    xs = [torch.randn(2, 3, 18, 18, device="cuda").to(BF16) for _ in range(3)]
    spec = "fp8_e4m3,qs=microscaling,bs=32"
    gm = qp.prepare_pt2e(m, qp.get_default_quantizer(input_activation=spec, weight=spec, force_scale_power_of_two=True), (xs[0],))
    with torch.no_grad():
        gm(xs[0])
        gm(xs[1])
        gc = qp.convert_pt2e(gm)
    target = torch.ops.quantized_ops.conv2d_mx.default
    seen = []

    class Recorder(torch.fx.Interpreter):
        def run_node(self, node):
            args, kwargs = self.fetch_args_kwargs_from_env(node)
            if node.op == "call_function" and node.target == target:
                before = mx_gemm.STATS.native
                had = mx_operand.operand_record(args[0], mx_operand.NHWC) is not None
                out = super().run_node(node)
                seen.append(dict(args=args, kwargs=kwargs, out=out, native=mx_gemm.STATS.native == before + 1, had=had))
                return out
            return super().run_node(node)

    mx_gemm.STATS.reset()
    with torch.no_grad():
        Recorder(gc).run(xs[2])
    assert len(seen) == 3 and [s["native"] for s in seen] == [False, True, True]           # the first layer has Cin = 3
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (2, 1)
    assert [s["had"] for s in seen] == [False, True, True]
    for s in seen[1:]:
        x, w, bias, stride, padding, dilation, groups = list(s["args"]) + [None, 1, 0, 1, 1][len(s["args"]) - 2:]
        kw = s["kwargs"]
        bs = kw["block_size"]
        dx, dw_ = dequantized64(x, kw["input_scale"], bs), dequantized64(w, kw["weight_scale"], bs)
        want = F.conv2d(dx, dw_, bias.cpu().double() if bias is not None else None, stride, padding, dilation).permute(0, 2, 3, 1)
        mag = F.conv2d(dx.abs(), dw_.abs(), None, stride, padding, dilation).permute(0, 2, 3, 1)
        within_bound(s["out"], want, mag, BF16, "converted CNN")
