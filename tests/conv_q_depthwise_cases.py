"""Shared by tests/test_conv_q_depthwise_cpu.py and tests/test_gpu_conv_q_depthwise.py: the depthwise cases, their exact fp64 sums, the
epilogue's rounding chain on the host, the converted inverted-residual block.  A plain module, imported by name; it holds no tests."""
import functools

import torch
import torch.nn.functional as F

BF16, F32 = torch.bfloat16, torch.float32

# (N, H, W, C, (kh, kw), stride, padding, dilation)
CASES = {
    "one_run": (2, 7, 7, 16, (3, 3), (1, 1), (1, 1), (1, 1)),              # one 16-channel run, a batch boundary
    "ragged_48": (2, 8, 9, 48, (3, 3), (2, 2), (1, 1), (1, 1)),            # ragged against a 32- or 64-channel slab, stride 2 on even and odd extents
    "five_144": (1, 9, 9, 144, (5, 5), (1, 1), (2, 2), (1, 1)),
    "seven_32": (1, 11, 11, 32, (7, 7), (2, 2), (3, 3), (1, 1)),           # 49 taps: two staging rounds of 32 taps
    "dilated_96": (2, 9, 7, 96, (3, 3), (1, 1), (2, 2), (2, 2)),           # dilation; corner pixels keep four of their nine taps
    "one_by_five": (1, 6, 8, 16, (1, 5), (1, 1), (0, 2), (1, 1)),
    "five_by_one": (1, 8, 6, 16, (5, 1), (1, 1), (2, 0), (1, 1)),
    "no_padding": (3, 5, 5, 16, (3, 3), (1, 1), (0, 0), (1, 1)),           # Ho Wo = 9, under any pixel tile
    "m128": (1, 9, 9, 16, (7, 7), (1, 1), (0, 0), (1, 1)),                 # all codes -128: 49 * 16384
    "pm127": (1, 6, 6, 32, (3, 3), (1, 1), (1, 1), (1, 1)),                # +-127, alternating signs
    "strip_plus_one": (1, 1, 257, 16, (3, 3), (1, 1), (1, 1), (1, 1)),     # one run: 256 pixels per workgroup, and one more
    "two_slabs": (1, 5, 5, 272, (3, 3), (1, 1), (1, 1), (1, 1)),           # a full 256-channel slab and a ragged one of one run
    "two_pixels": (2, 64, 64, 512, (3, 3), (1, 1), (1, 1), (1, 1)),        # N Ho Wo C / 16 = 2^18: the two-pixels-per-thread variant
}
FIRST_FIVE = list(CASES)[:5]


def out_hw(case):
    n, h, w, c, (kh, kw), (sh, sw), (ph, pw), (dh, dw) = CASES[case]
    return (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def dw_exact(xq, wq, stride, padding, dilation):
    """xq [N, C, H, W], wq [C, 1, kh, kw] integer-valued -> the exact sums in fp64, NHWC rows [N, Ho Wo, C].  Every product and sum is an
    integer far below 2^53, so the fp64 grouped convolution is exact in any order."""
    y = F.conv2d(xq.double(), wq.double(), None, stride, padding, dilation, xq.shape[1])
    return y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, y.shape[1]).contiguous()


def fold32(v):
    """The identity value map on an fp32 tensor: the high 16 bits with a sticky bit."""
    pre = v.contiguous().view(torch.int32)
    return ((pre & -65536) | ((pre & 0xFFFF) != 0).int() * 65536).view(torch.float32)


def chain(exact, bias, s, dtype, fold):
    """The rounding chain of the epilogue on the host.  exact fp64 [..., C]; bias / s in `dtype` ([C] / [1] or [C]) or None."""
    v = exact.float()                                             # |sum| < 2^24: exact
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
    """Codes (x NHWC int8, w [C, kh, kw] int8, and the integer-valued NCHW / [C, 1, kh, kw] tensors), the exact sums, a bias and
    per-channel factors.  Computed once per case and shared: callers leave them unchanged."""
    n, h, w, c, (kh, kw), stride, padding, dilation = CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    if case == "m128":
        xq, wq = torch.full((n, c, h, w), -128), torch.full((c, 1, kh, kw), -128)
    elif case == "pm127":
        sx = 1 - 2 * ((torch.arange(h).view(h, 1) + torch.arange(w).view(1, w)) % 2)      # a checkerboard, like the 3 x 3 filter's
        xq = (127 * sx).view(1, 1, h, w).expand(n, c, h, w).contiguous()
        wq = (127 * torch.tensor([1, -1, 1, -1, 1, -1, 1, -1, 1]).view(1, 1, kh, kw) * torch.tensor([1, -1] * (c // 2)).view(c, 1, 1, 1)).contiguous()
    else:
        xq = torch.randint(-128, 128, (n, c, h, w), generator=g)
        wq = torch.randint(-128, 128, (c, 1, kh, kw), generator=g)
    exact = dw_exact(xq, wq, stride, padding, dilation)
    bias = torch.randint(-3000, 3000, (c,), generator=g).float()
    scale = torch.rand(c, generator=g) * 1e-3 + 1e-4
    return dict(xq=xq, wq=wq, x=xq.permute(0, 2, 3, 1).contiguous().to(torch.int8), w=wq.reshape(c, kh, kw).contiguous().to(torch.int8),
                exact=exact, bias=bias, scale=scale)


def ulp(v, dtype):
    """One rounding step of `dtype` at magnitude v (fp64 tensor)."""
    mant = 7 if dtype == BF16 else 23
    e = torch.floor(torch.log2(v.clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def layer_bound(exact, abs_exact, k, b, out_scale, dtype):
    """tests/test_gpu_conv_q.py's bound with the exact sums handed in: the fp32 accumulation of the value-tensor convolution is within
    k 2^-24 sum|q_x||q_w| of the exact sum (k = kh kw for a depthwise layer, Cin for a pointwise one); one rounding step of the output
    dtype at each of the two rounding points (a library convolution may round the sum before it adds the bias and again behind the
    add: one step at the larger magnitude covers both); scaled by |s|.  exact, abs_exact fp64 [N, L, C] -> (exact result, bound)."""
    acc = k * 2.0 ** -24 * abs_exact
    v = exact + (b.cpu().double() if b is not None else 0.0)
    s = out_scale.cpu().double().reshape(-1)
    first = acc + ulp(torch.maximum(exact.abs(), v.abs()) + acc, dtype)
    return v * s, first * s.abs() + ulp((v.abs() + first) * s.abs(), dtype)


class Block(torch.nn.Module):
    """A MobileNetV2-style inverted residual block behind a stem: 3 -> 16 (3 x 3, stays aten.conv2d), expand 16 -> 96 (1 x 1), depthwise
    96 (3 x 3, stride 2), project 96 -> 32 (1 x 1)."""

    def __init__(self):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, 16, 3, padding=1)
        self.expand = torch.nn.Conv2d(16, 96, 1)
        self.dw = torch.nn.Conv2d(96, 96, 3, stride=2, padding=1, groups=96)
        self.project = torch.nn.Conv2d(96, 32, 1)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        x = torch.relu(self.expand(x))
        x = torch.relu(self.dw(x))
        return self.project(x)


SPEC = "int8,qs=per_tensor_symmetric"


def convert_block(dtype, device="cpu", native=False, net=None, x=None):
    """prepare_pt2e / convert_pt2e of `net` (the block by default) under the ImageNet recipe's specs -> (graph module, input)."""
    from quantized_training import quantize_pt2e as qp
    if x is None:
        torch.manual_seed(3)
        x = torch.randn(2, 3, 12, 12)
    x = x.to(dtype).to(device)
    torch.manual_seed(4)
    net = (net if net is not None else Block()).to(device).to(dtype).eval()
    gm = qp.prepare_pt2e(net, qp.get_default_quantizer(SPEC, None, SPEC, "int24"), (x,))
    with torch.no_grad():
        gm(x), gm(x * 0.5)
    return qp.convert_pt2e(gm, native=native), x
