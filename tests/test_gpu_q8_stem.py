"""The stem convolution of converted per-tensor int8 CNNs on the device: qt_q8_stem_conv2d / _codes and qt_quantize_codes_nhwc4_* through
the C ABI, the operator quantized_ops.conv2d_q on its stem route, a converted three-layer CNN and its graph capture.

Exact tier: the reference is the fp64 convolution of the integer codes on the host (every sum is an integer of magnitude <= 2^24:
exact) pushed through the stated rounding chain; the device result must equal it bit for bit.  Operands sit between margins of 0xFF
(-1 as a code: a read outside an operand changes a sum), outputs between margins of NaN."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_q_depthwise_cases as K
from conv_q_depthwise_cases import BF16, F32
from kernel_launch import nv, stream  # noqa: F401

pytestmark = pytest.mark.gpu

#        N Cin  H   W  Cout  kh  kw  stride  pad
ROWS = [(2, 3, 21, 21, 64, 7, 7, 2, (3, 3)),       # ragged patches on both axes, two images
        (1, 3, 9, 13, 32, 3, 3, 2, (1, 1)),        # K below one k step
        (1, 1, 8, 8, 16, 5, 5, 1, (2, 2)),
        (1, 4, 10, 10, 48, 3, 3, 1, (0, 0)),       # ragged column tile
        (1, 2, 12, 12, 144, 3, 3, 1, (1, 1)),      # second column tile
        (1, 3, 35, 35, 64, 11, 11, 4, (2, 2)),
        (1, 3, 8, 20, 16, 1, 7, 1, (0, 3)),
        (1, 3, 20, 8, 16, 7, 1, 1, (3, 0)),
        (1, 3, 6, 6, 16, 3, 3, 1, (4, 4)),         # padding wider than the filter
        (1, 3, 7, 7, 16, 7, 7, 1, (0, 0)),         # one output pixel
        (1, 4, 10, 10, 64, 4, 4, 1, (1, 1)),       # all codes -128 x all weights -128, the largest sum
        (1, 3, 9, 10, 32, 3, 3, 3, (1, 1))]        # stride 3
LARGEST = 10
PAD = 256


@functools.lru_cache(maxsize=None)
def operands(i):
    """Shared, never modified: integer-valued xq [N, Cin, H, W], wq [Cout, Cin, kh, kw], the exact sums as NHWC rows, bias, factors."""
    n, cin, h, w, cout, kh, kw, st, pad = ROWS[i]
    g = torch.Generator().manual_seed(100 + i)
    xq, wq = torch.randint(-128, 128, (n, cin, h, w), generator=g), torch.randint(-128, 128, (cout, cin, kh, kw), generator=g)
    xq.view(-1)[0] = wq.view(-1)[0] = -128
    if i == LARGEST:
        xq, wq = torch.full_like(xq, -128), torch.full_like(wq, -128)
    y = F.conv2d(xq.double(), wq.double(), None, st, pad)
    exact = y.permute(0, 2, 3, 1).reshape(n, -1, cout).contiguous()
    x4 = torch.zeros(n, h, w, 4, dtype=torch.int8)
    x4[..., :cin] = xq.permute(0, 2, 3, 1).to(torch.int8)
    return dict(xq=xq, wq=wq, exact=exact, x4=x4, w=wq.permute(0, 2, 3, 1).contiguous().to(torch.int8), ho=y.shape[2], wo=y.shape[3],
                bias=torch.randint(-3000, 3000, (cout,), generator=g).float(), scale=torch.rand(cout, generator=g) * 1e-3 + 1e-4)


def between_margins(host, fill):
    """host bytes on the device between two margins of `fill` -> (whole buffer, 16-byte aligned pointer to the payload)."""
    host = host.contiguous().view(torch.uint8).reshape(-1)
    raw = torch.full((host.numel() + 2 * PAD,), fill, dtype=torch.uint8, device="cuda")
    raw[PAD:PAD + host.numel()] = host.cuda()
    assert (raw.data_ptr() + PAD) % 16 == 0
    return raw, raw.data_ptr() + PAD


def stem(nv, i, dtype, bias, s, per_col, fold, tail=None):
    """One launch of the entry (tail: the _codes sibling's trailing arguments) -> y [N, Ho Wo, Cout] on the host; status 0, the
    operands and their margins unchanged, the output's margins unwritten."""
    n, cin, h, w, cout, kh, kw, st, (ph, pw) = ROWS[i]
    o = operands(i)
    (xr, xp), (wr, wp) = between_margins(o["x4"], 0xFF), between_margins(o["w"], 0xFF)
    images = xr.clone(), wr.clone()
    count, out_dtype = n * o["ho"] * o["wo"] * cout, dtype if tail is None else torch.int8
    esz = torch.empty(0, dtype=out_dtype).element_size()
    buf = torch.full((count * esz + 2 * PAD,), 0xFF, dtype=torch.uint8, device="cuda")          # 0xFFFF / 0xFFFFFFFF are NaNs
    b, sd = (t.to(dtype).cuda() if t is not None else None for t in (bias, s))
    args = (xp, wp, buf.data_ptr() + PAD, int(dtype == F32), b.data_ptr() if b is not None else None,
            sd.data_ptr() if sd is not None else None, per_col, fold, n, h, w, cin, cout, kh, kw, st, st, ph, pw, 1, 1)
    fn = nv.lib().qt_q8_stem_conv2d if tail is None else nv.lib().qt_q8_stem_conv2d_codes
    assert fn(*args, *(tail or ()), stream()) == 0
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:PAD] == 0xFF).all()) and bool((host[PAD + count * esz:] == 0xFF).all()), f"row {i}: a margin of y was written"
    assert torch.equal(xr, images[0]) and torch.equal(wr, images[1]), f"row {i}: an operand changed"
    return host[PAD:PAD + count * esz].view(out_dtype).reshape(n, -1, cout)


def same_bits(got, want, what):
    bits = {BF16: torch.int16, F32: torch.int32, torch.int8: torch.int8}[got.dtype]
    bad = got.contiguous().view(bits) != want.contiguous().view(bits)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("i", range(len(ROWS)))
def test_stem_is_exact(nv, i):
    """bf16 output with a scalar factor; fp32 output with per-channel factors, bias and the identity fold."""
    o = operands(i)
    if i == LARGEST:
        assert float(o["exact"].max()) == 4 * 4 * 4 * 16384
    s16 = o["scale"][:1].bfloat16()
    same_bits(stem(nv, i, BF16, None, s16, 0, 0), K.chain(o["exact"], None, s16, BF16, 0), f"row {i} bf16")
    same_bits(stem(nv, i, F32, o["bias"], o["scale"], 1, 1), K.chain(o["exact"], o["bias"], o["scale"], F32, 1), f"row {i} fp32")


def int8_map():
    import quantized_training as qt
    return qt.get_quantization_map("int8", torch.device("cuda"))


@pytest.mark.parametrize("i,dtype", [(0, BF16), (3, F32), (4, BF16)])
def test_codes_sibling_equals_the_value_sibling_quantized(nv, i, dtype):
    """_codes on three rows (64, ragged 48, 144 columns): the value sibling's bits, clamped to [0, 6] in the model dtype, through
    qt_quantize_codes_nhwc_*."""
    o, qmap = operands(i), int8_map()
    bias, s = o["bias"].to(dtype), o["scale"].to(dtype)
    next_scale = torch.tensor([0.05]).to(dtype).cuda()
    y = stem(nv, i, dtype, bias, s, 1, 0)
    got = stem(nv, i, dtype, bias, s, 1, 0, tail=(1, 0.0, 6.0, next_scale.data_ptr(), qmap.data_ptr()))
    from quantized_training.pt2e_native import conv_codes_nhwc
    values = y.clamp(0.0, 6.0).view(y.shape[0], o["ho"], o["wo"], -1).permute(0, 3, 1, 2).cuda()              # channels_last
    same_bits(got, conv_codes_nhwc(values, next_scale, qmap).view(got.shape).cpu(), f"row {i} codes")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_nhwc4_pass_equals_quantize_and_narrow(nv, dtype, c):
    """Both layouts, with NaN and +-inf planted: byte ch of a pixel's dword = narrow(quantize(x)), the bytes >= C zero."""
    from quantized_training import pt2e_native
    x = (torch.randn(2, c, 7, 9, generator=torch.Generator().manual_seed(c)) * 3).to(dtype)
    x.view(-1)[:3] = torch.tensor([float("nan"), float("inf"), float("-inf")]).to(dtype)
    scale, qmap = torch.tensor(0.04).to(dtype).cuda(), int8_map()
    want = torch.zeros(2, 7, 9, 4, dtype=torch.int8)
    want[..., :c] = pt2e_native._narrow_codes(torch.ops.quantized_ops.quantize(x.cuda(), scale, None, None, None, qmap)).permute(0, 2, 3, 1).cpu()
    for xin in (x.cuda(), x.cuda().contiguous(memory_format=torch.channels_last)):
        same_bits(pt2e_native.conv_codes_nhwc(xin, scale, qmap, stem=True).cpu().view(2, 7, 9, 4), want, f"nhwc4 C = {c}")


def test_refusals_leave_the_output_alone(nv):
    """Every refusal of the contract with device pointers: answered before a launch, the buffer keeps its sentinel."""
    from test_q8_stem_cpu import check_refusals
    buf = torch.full((1 << 14,), float("nan"), dtype=F32, device="cuda")
    check_refusals(nv.lib(), buf.data_ptr(), stream())
    torch.cuda.synchronize()
    assert bool(buf.isnan().all())


def op_args(dtype, marked):
    from quantized_training import pt2e_native
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(2, 3, 19, 17, generator=g) * 2).to(dtype).cuda()
    wc = torch.randint(-127, 128, (32, 5, 5, 3), generator=g).to(torch.int8).cuda()
    b = torch.randint(-4000, 4000, (32,), generator=g).to(dtype).cuda()
    out_scale = (torch.rand(32, 1, 1, generator=g) * 1e-3 + 1e-4).to(dtype).cuda()
    return x, torch.tensor(0.04).to(dtype).cuda(), int8_map(), pt2e_native.mark_stem(wc) if marked else wc, b, [2, 2], [2, 2], [1, 1], 1, out_scale


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_operator_marked_is_exact_and_unmarked_declines_as_before(nv, monkeypatch, dtype):
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    monkeypatch.setattr(pt2e_native, "CONV_Q_REASONS", {})
    args = op_args(dtype, True)
    x, scale, qmap, wc, b = args[:5]
    xq = torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap).cpu()
    exact = F.conv2d(xq.double(), wc.cpu().permute(0, 3, 1, 2).double(), None, 2, 2).permute(0, 2, 3, 1).reshape(2, -1, 32)
    before = dict(pt2e_native.STATS)
    for xin in (x, x.contiguous(memory_format=torch.channels_last)):
        y = torch.ops.quantized_ops.conv2d_q(xin, *args[1:], None, "int8")
        assert y.shape == (2, 32, 10, 9) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
        same_bits(y.permute(0, 2, 3, 1).reshape(2, -1, 32).cpu(), K.chain(exact, b.cpu(), args[-1].cpu().reshape(-1), dtype, 0), f"operator {dtype}")
    assert pt2e_native.STATS == {**before, "conv2d_stem_int8": before["conv2d_stem_int8"] + 2} and not pt2e_native.CONV_Q_REASONS
    torch.ops.quantized_ops.conv2d_q(*op_args(dtype, False), None, "int8")                                   # no mark: today's decline
    assert pt2e_native.CONV_Q_REASONS == {"Cin = 3 / 3: not a multiple of 32": 1}


class Net(torch.nn.Module):
    """stem 3 -> 32 (3 x 3 / 2) -> ReLU6 -> depthwise 3 x 3 -> ReLU6 -> pointwise 32 -> 16."""

    def __init__(self):
        super().__init__()
        self.stem, self.dw, self.pw = torch.nn.Conv2d(3, 32, 3, 2, 1), torch.nn.Conv2d(32, 32, 3, 1, 1, groups=32), torch.nn.Conv2d(32, 16, 1)

    def forward(self, x):
        return self.pw(F.hardtanh(self.dw(F.hardtanh(self.stem(x), 0.0, 6.0)), 0.0, 6.0))


class PerLayer(torch.fx.Interpreter):
    """Every conv2d_q / conv2d_qc node against the same operator on the host, which runs the graph's three nodes (and the activation
    and the consumer's quantize of a codes-out node) verbatim, on the node's own inputs: the same bits."""
    checked = 0

    def call_function(self, target, args, kwargs):
        out = super().call_function(target, args, kwargs)
        if "conv2d_q" in str(target):
            want = target(*[a.cpu() if isinstance(a, torch.Tensor) else a for a in args])
            assert out.dtype == want.dtype
            same_bits(out.cpu(), want, f"layer {target} {tuple(args[3].shape)}")
            self.checked += 1
        return out


@pytest.mark.parametrize("setting", [{}, {"native_stem": True}, {"native_stem": True, "chain_convs": True}], ids=["default", "stem", "stem_chain"])
def test_converted_cnn(nv, monkeypatch, setting):
    """The default graph keeps the stem as aten.conv2d; every native layer gives the bits of the graph's own nodes on the host (integer
    sums below 2^24 are exact in fp32 in any order, the roundings are the same), and with native_stem so does the whole model; the
    capture replays the eager bits."""
    from quantized_training import pt2e_native, quantize_pt2e as qp
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    torch.manual_seed(3)
    x = torch.randn(2, 3, 21, 19).to(BF16).cuda()
    torch.manual_seed(4)
    gm = qp.prepare_pt2e(Net().cuda().to(BF16).eval(), qp.get_default_quantizer(K.SPEC, None, K.SPEC, "int24"), (x,))
    with torch.no_grad():
        gm(x), gm(x * 0.5)
        ref = qp.convert_pt2e(__import__("copy").deepcopy(gm), native=False).cpu()
        g = qp.convert_pt2e(gm, native=True, **setting)
    t = [str(n.target) for n in g.graph.nodes if n.op == "call_function"]
    assert t.count("aten.conv2d.default") == (0 if setting else 1) and any("conv2d_q" in s for s in t)
    assert sum("conv2d_qc" in s for s in t) == (3 if "chain_convs" in setting else 0)
    before = dict(pt2e_native.STATS)
    with torch.no_grad():
        y, want = g(x).clone(), ref(x.cpu())
    ran = {k: pt2e_native.STATS[k] - before[k] for k in before}
    assert ran["conv2d_stem_int8"] == int(bool(setting)) and ran["conv2d_dw_int8"] == 1 and ran["conv2d_int8"] == 1, ran
    assert ran["conv2d_codes_out"] == ran["conv2d_codes_in"] == 2 * int("chain_convs" in setting)
    with torch.no_grad():
        layers = PerLayer(g)
        layers.run(x)
    assert layers.checked == (3 if setting else 2)
    if setting:
        same_bits(y.cpu(), want, f"converted CNN {setting}")
        static_x = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            g(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            out = g(static_x)
        for _ in range(3):
            static_x.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            same_bits(out.cpu(), y.cpu(), "replay")
