"""Shared by tests/test_conv_q_splitk_cpu.py and tests/test_gpu_conv_q_splitk.py: the problems of the split-K int8 convolution
(qt_q8_conv2d_ws / qt_q8_conv2d_codes_ws, csrc/qt_mx_conv.hip), their exact sums and the epilogue's rounding chain on the host
(restated from tests/test_gpu_conv_q.py), and the small converted CNN with a projecting 1 x 1 layer.  A plain module, imported by
name; it holds no tests."""
import functools

import torch
import torch.nn.functional as F

BF16, F32 = torch.bfloat16, torch.float32
SLAB = 65536                     # workspace bytes per tile and split: 128 x 128 int32

# name -> ((N, H, W, Cin, Cout, (kh, kw), stride, padding, dilation), the forced splits)
CASES = {
    # 1 x 1, nk = 2: one k tile per split; M = 25 and Cout = 48: ragged rows and columns
    "one_tile_each": ((1, 5, 5, 256, 48, (1, 1), (1, 1), (0, 0), (1, 1)), (2,)),
    # K = 288, nk = 3 with a 32-byte tail.  S = 2: the second split starts at k tile 1 = tap (1, 1), inside a tap row; S = 3: the
    # last split owns only the tail tile
    "starts_in_tap_row": ((1, 5, 5, 32, 16, (3, 3), (1, 1), (1, 1), (1, 1)), (2, 3)),
    # Cin = 96: cpb = 3, K = 864, nk = 7: splits start at 32-block 1 or 2 of a pixel (u_blk != 0); uneven ranges
    "mid_pixel_stride": ((2, 9, 9, 96, 144, (3, 3), (2, 2), (0, 0), (1, 1)), (2, 4, 7)),
    "mid_pixel_dilation": ((2, 9, 9, 96, 144, (3, 3), (1, 1), (2, 2), (2, 2)), (2, 4, 7)),
    # nk = 8, M = 200, Cout = 144: four tiles with eight tickets each, two of them ragged each way
    "four_tiles": ((2, 10, 10, 1024, 144, (1, 1), (1, 1), (0, 0), (1, 1)), (8,)),
    # +-127 codes with one 126: odd sums above 2^24 -- the partial sums must be added as integers in front of the one conversion
    "pm127_odd": ((1, 4, 4, 128, 8, (3, 3), (1, 1), (1, 1), (1, 1)), (4,)),
    # every code -128, kh kw Cin = 2^17 - 32: the largest sum the entry point admits, no wrap in a partial or in the total
    "m128_longest": ((1, 3, 3, 14560, 8, (3, 3), (1, 1), (1, 1), (1, 1)), (8,)),
}


def geometry(case):
    n, h, w, cin, cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw) = CASES[case][0]
    return (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def tiles_nk(case):
    n, h, w, cin, cout, (kh, kw), *_ = CASES[case][0]
    ho, wo = geometry(case)
    return -(-n * ho * wo // 128) * -(-cout // 128), -(-kh * kw * cin // 128)


def conv_exact(xq, wq, stride, padding, dilation):
    """xq [N, Cin, H, W], wq [Cout, Cin, kh, kw] integer-valued -> the exact sums, fp64 NHWC [N, Ho Wo, Cout] (unfold + matmul)."""
    cout = wq.shape[0]
    cols = F.unfold(xq.double(), wq.shape[2:], dilation, padding, stride)
    return torch.matmul(wq.double().reshape(cout, -1), cols).transpose(1, 2).contiguous()


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
    """Codes (int8 NHWC / [Cout, kh, kw, Cin]), the exact sums, a bias and per-channel factors: computed once, left unchanged."""
    n, h, w, cin, cout, (kh, kw), stride, padding, dilation = CASES[case][0]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    if case == "pm127_odd":
        sign = (torch.randint(0, 2, (cin,), generator=g) * 2 - 1)
        xq = (127 * sign).view(1, cin, 1, 1).expand(n, cin, h, w).contiguous()
        wsign = torch.tensor([1, -1] * (cout // 2)).view(cout, 1, 1, 1)
        wq = ((127 * sign).view(1, cin, 1, 1) * wsign).expand(cout, cin, kh, kw).contiguous()
        wq[:, 0, 1, 1] = wq[:, 0, 1, 1] // 127 * 126              # the centre tap: inside every output pixel's window
    elif case == "m128_longest":
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


def int8_map(device="cpu"):
    import quantized_training as qt
    return qt.get_quantization_map("int8", torch.device(device))


class ProjectNet(torch.nn.Module):
    """A stem over 3 channels (stays aten.conv2d), an expanding 1 x 1 layer to 1024 channels and a PROJECTING 1 x 1 layer 1024 -> 32
    (Cout < Cin, nk = 8, four row tiles: the class the split is for), a Linear head."""

    def __init__(self):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, 32, 3, padding=1)
        self.expand = torch.nn.Conv2d(32, 1024, 1)
        self.project = torch.nn.Conv2d(1024, 32, 1)
        self.fc = torch.nn.Linear(32, 10)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        x = torch.relu(self.expand(x))
        x = self.project(x)
        return self.fc(x.mean((2, 3)))


def convert_project_net(monkeypatch, device, **convert_kw):
    """ProjectNet prepared, calibrated and converted with QT_PT2E_NATIVE=1 and the given convert_pt2e keywords -> (graph, input)."""
    from quantized_training import quantize_pt2e as qp
    monkeypatch.setenv("QT_PT2E_NATIVE", "1")
    torch.manual_seed(3)
    x = torch.randn(4, 3, 10, 10).bfloat16().to(device)
    torch.manual_seed(4)
    net = ProjectNet().to(device).bfloat16().eval()
    spec = "int8,qs=per_tensor_symmetric"
    gm = qp.prepare_pt2e(net, qp.get_default_quantizer(spec, None, spec, "int24"), (x,))
    with torch.no_grad():
        gm(x), gm(x * 0.5)
    return qp.convert_pt2e(gm, **convert_kw), x


def call_targets(gm):
    return [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
