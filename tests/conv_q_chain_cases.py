"""Shared by tests/test_conv_q_chain_cpu.py and tests/test_gpu_conv_q_chain.py: the problems of the codes-out kernels, their expected
codes from the host reference (exact fp64 sums -> the epilogue's rounding chain -> torch.clamp -> CPU quantized_ops.quantize, narrowed),
the non-vacuity of those expectations, the converted blocks.  A plain module, imported by name; it holds no tests."""
import functools

import torch
import torch.nn.functional as F

import conv_q_depthwise_cases as K
from conv_q_depthwise_cases import BF16, F32

# Activation settings: name -> (bounds or None, sigma, next_scale).  sigma is the standard deviation the dequantize factor gives the
# values; with it and next_scale the expected codes hold a saturated code, a zero and (with a clamp) elements at both bounds:
#   next_scale 0.01 at sigma 1: |v| >= 1.28 saturates, |v| < 0.005 is code 0 (0.4 % of the elements);
#   hardtanh(0, 6) at sigma 4: 6.7 % of the elements sit at 6 = code 127 at next_scale 0.04, the negative half at 0;
#   (-1.5, 2.25) are bf16 values: -1.5 / 0.0117 < -128; (-1.3, 1.1) are not (the clamp's result is the bound rounded to bf16).
ACTS = {
    "none": (None, 1.0, 0.01),
    "relu": ((0.0, None), 1.0, 0.01),
    "hardtanh_0_6": ((0.0, 6.0), 4.0, 0.04),
    "hardtanh_bf16_bounds": ((-1.5, 2.25), 1.0, 0.0117),
    "hardtanh_rounded_bounds": ((-1.3, 1.1), 1.0, 0.01),
}
SIGMA_PRODUCT = ((256 ** 2 - 1) / 12.0)          # variance of a uniform int8 code = standard deviation of a product of two

# gather kernel: Cin = 32, 3 x 3, stride 2, padding 1.  (N, H, W) -> M = N Ho Wo
GATHER_M = {126: (2, 14, 18), 130: (2, 10, 26)}     # one ragged row tile; a second tile holding two rows
GATHER_COUT = (16, 48, 144)                          # one run; one wave's 64-column half partly empty; a second column tile of one run
# depthwise kernel: (N, H, W, C, stride); the last two straddle the two-pixels-per-thread switch (M C / 16 = 2 * 64 * 2048)
DW = {
    "c16_s1": (2, 9, 9, 16, 1), "c16_s2": (2, 9, 9, 16, 2), "c48_s1": (2, 8, 9, 48, 1), "c48_s2": (2, 8, 9, 48, 2),
    "c272_s1": (1, 5, 5, 272, 1), "c272_s2": (1, 9, 9, 272, 2),
    "one_pixel": (1, 124, 124, 272, 1), "two_pixels": (1, 124, 125, 272, 1),
}
DW_BIG = ("one_pixel", "two_pixels")
# pointwise GEMM: M = 130
GEMM_K, GEMM_N, GEMM_M = (16, 48, 144), (16, 144), 130


def int8_map(device="cpu"):
    import quantized_training as qt
    return qt.get_quantization_map("int8", torch.device(device))


def narrow(v):
    """A quantize node's values -> int8 as the device's code_of narrows them: NaN -> 0, saturate, truncate."""
    return torch.nan_to_num(v.float(), nan=0.0, posinf=127.0, neginf=-128.0).clamp(-128.0, 127.0).to(torch.int8)


def clamp(v, bounds):
    return v if bounds is None else torch.clamp(v, min=bounds[0], max=bounds[1])


def expected_codes(exact, bias, s, dtype, fold, bounds, next_scale):
    """exact fp64 [..., C] -> the int8 codes the chained kernel must write, and the values in front of the quantize."""
    qmap = int8_map()                                         # imports the package, which registers quantized_ops
    v = clamp(K.chain(exact, bias, s, dtype, fold), bounds)
    q = torch.ops.quantized_ops.quantize(v, torch.tensor(next_scale).to(dtype), None, None, None, qmap)
    return narrow(q), v


def assert_not_vacuous(codes, v, bounds, what):
    c = codes.reshape(-1).long()
    assert bool(((c == -128) | (c == 127)).any()), f"{what}: no saturated code expected"
    assert bool((c == 0).any()), f"{what}: no zero code expected"
    assert c.unique().numel() >= 32, f"{what}: {c.unique().numel()} distinct codes expected"
    if bounds is not None:
        for b in bounds:
            if b is not None:
                assert bool((v.float() == torch.tensor(b).to(v.dtype).float()).any()), f"{what}: the bound {b} binds nowhere"


def factors(cout, k, sigma, per_channel, dtype, seed):
    """A bias of about half a standard deviation of the sums and the dequantize factor(s) that give the values `sigma`."""
    g = torch.Generator().manual_seed(seed)
    sd = SIGMA_PRODUCT * k ** 0.5
    bias = (torch.randint(-int(sd / 2), int(sd / 2), (cout,), generator=g)).float().to(dtype)
    s = sigma / sd * ((0.5 + torch.rand(cout, generator=g)) if per_channel else torch.ones(1))
    return bias, s.to(dtype)


@functools.lru_cache(maxsize=None)
def gather_operands(m, cout):
    n, h, w = GATHER_M[m]
    g = torch.Generator().manual_seed(1000 * m + cout)
    xq = torch.randint(-128, 128, (n, 32, h, w), generator=g)
    wq = torch.randint(-128, 128, (cout, 32, 3, 3), generator=g)
    y = F.conv2d(xq.double(), wq.double(), None, 2, 1)
    exact = y.permute(0, 2, 3, 1).reshape(-1, cout).contiguous()
    assert exact.shape[0] == m
    return dict(x=xq.permute(0, 2, 3, 1).contiguous().to(torch.int8), w=wq.permute(0, 2, 3, 1).contiguous().to(torch.int8), exact=exact, k=288)


@functools.lru_cache(maxsize=None)
def dw_operands(case):
    n, h, w, c, s = DW[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    xq = torch.randint(-128, 128, (n, c, h, w), generator=g)
    wq = torch.randint(-128, 128, (c, 1, 3, 3), generator=g)
    exact = K.dw_exact(xq, wq, s, 1, 1).reshape(-1, c)
    return dict(x=xq.permute(0, 2, 3, 1).contiguous().to(torch.int8), w=wq.reshape(c, 3, 3).contiguous().to(torch.int8), exact=exact, k=9)


@functools.lru_cache(maxsize=None)
def gemm_operands(k, n):
    g = torch.Generator().manual_seed(100 * k + n)
    a = torch.randint(-128, 128, (GEMM_M, k), generator=g)
    b = torch.randint(-128, 128, (n, k), generator=g)
    return dict(x=a.to(torch.int8), w=b.to(torch.int8), exact=a.double() @ b.double().t(), k=k)


def settings(big=False):
    """(dtype, per-channel factor, bias, activation) of the exact tier; two of them for the two large depthwise problems."""
    if big:
        return [(BF16, True, True, "hardtanh_0_6"), (F32, False, False, "relu")]
    return [(d, pc, hb, act) for d in (BF16, F32) for pc in (False, True) for hb in (False, True) for act in ACTS]


@functools.lru_cache(maxsize=None)
def expectation(family, key, dtype, per_channel, has_bias, act):
    """The arguments and the expected codes of one exact case, vacuity checked: computed once and shared; callers leave them unchanged."""
    ops = {"gather": gather_operands, "dw": dw_operands, "gemm": gemm_operands}[family](*key)
    bounds, sigma, next_scale = ACTS[act]
    cout = ops["exact"].shape[-1]
    bias, s = factors(cout, ops["k"], sigma, per_channel, dtype, seed=cout + 7 * per_channel)
    bias = bias if has_bias else None
    fold = int(dtype == F32 and per_channel)                 # the fp32 identity fold rides along with the per-channel factor
    codes, v = expected_codes(ops["exact"], bias, s, dtype, fold, bounds, next_scale)
    assert_not_vacuous(codes, v, bounds, f"{family} {key} {dtype} {per_channel} {has_bias} {act}")
    return dict(ops=ops, bias=bias, s=s, fold=fold, bounds=bounds, next_scale=torch.tensor([next_scale]).to(dtype), codes=codes)


def tail_args(bounds):
    """(act, act_lo, act_hi) of the C entry points."""
    if bounds is None:
        return 0, 0.0, 0.0
    return 1, float("-inf") if bounds[0] is None else bounds[0], float("inf") if bounds[1] is None else bounds[1]


class Block6(torch.nn.Module):
    """conv_q_depthwise_cases.Block with nn.ReLU6 behind every layer: the converted graph holds aten.hardtanh(., 0.0, 6.0)."""

    def __init__(self):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, 16, 3, padding=1)
        self.expand = torch.nn.Conv2d(16, 96, 1)
        self.dw = torch.nn.Conv2d(96, 96, 3, stride=2, padding=1, groups=96)
        self.project = torch.nn.Conv2d(96, 32, 1)
        self.act = torch.nn.ReLU6()

    def forward(self, x):
        x = self.act(self.stem(x))
        x = self.act(self.expand(x))
        x = self.act(self.dw(x))
        return self.project(x)


def seeded(net_cls):
    """The network with the weights conv_q_depthwise_cases.convert_block gives its own default: two conversions hold the same model."""
    torch.manual_seed(4)
    return net_cls()


def call_targets(gm):
    return [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
