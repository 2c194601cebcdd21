"""The block-scaled operand hand-over on the device: a tensor written in place between quantize_mx and linear_mx / matmul_mx / conv2d_mx.

What quantize_mx left on its results (format, power-of-two flag, packed operand: quantized_training/mx_operand.py) describes the
tensor as it was.  After `q.neg_()` or `s.mul_(2)` the record is stale, the operator takes the composite on the MODIFIED tensors --
bit for bit the composite restated here -- and counts a fallback.  Every case first runs the untouched call (native) and requires the
modified call's result to differ from it, so that no case can pass vacuously.  A weight is another matter: its packed operand is
cached under a key that carries both version counters, so a written-to weight is packed again, with the packer's check on, and the
call stays native on the new values.  Inference tensors have no version counter: there the native route stays."""
import pytest
import torch
import torch.nn.functional as F

from kernel_launch import nv  # noqa: F401

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FMT, QMAX, BS = "fp8_e4m3", 448.0, 32
CONV = dict(stride=[1, 1], padding=[1, 1], dilation=[1, 1])        # test_gpu_conv_mx's case A: 1 x 32 x 5 x 5 -> 16, 3 x 3


def bits_of(t):
    return t.detach().contiguous().view(torch.int16)


def quantized(t, axis):
    from quantized_training.fake_quantize import get_quantization_map
    s, q = torch.ops.quantized_ops.quantize_mx(t, get_quantization_map(FMT, "cuda"), [axis], BS, QMAX, True, None, None)
    return q, s


def sources():
    g = torch.Generator().manual_seed(21)
    r = lambda *shape: torch.randn(*shape, generator=g).to(BF16).cuda()                      # noqa: E731
    return {"linear_mx": (r(96, 64), r(80, 64)), "matmul_mx": (r(3, 96, 64), r(3, 64, 80)),
            "conv2d_mx": ((r(1, 32, 5, 5) * 2).contiguous(memory_format=torch.channels_last), r(16, 32, 3, 3) * 0.5)}


# op -> (block axis of the first / the second operand, the call, the composite of decomposed.py restated)
OPS = {
    "linear_mx": (-1, -1,
                  lambda a, b, sa, sb: torch.ops.quantized_ops.linear_mx(a, b, None, input_scale=sa, weight_scale=sb, block_size=BS),
                  lambda a, b, sa, sb: F.linear(a * sa.repeat_interleave(BS, -1), b * sb.repeat_interleave(BS, -1), None)),
    "matmul_mx": (-1, -2,
                  lambda a, b, sa, sb: torch.ops.quantized_ops.matmul_mx(a, b, input_scale=sa, weight_scale=sb, block_size=BS),
                  lambda a, b, sa, sb: torch.matmul(a * sa.repeat_interleave(BS, -1), b * sb.repeat_interleave(BS, -2))),
    "conv2d_mx": (1, 1,
                  lambda a, b, sa, sb: torch.ops.quantized_ops.conv2d_mx(a, b, None, CONV["stride"], CONV["padding"], CONV["dilation"], 1,
                                                                         input_scale=sa, weight_scale=sb, block_size=BS),
                  lambda a, b, sa, sb: F.conv2d(a * sa.repeat_interleave(BS, 1), b * sb.repeat_interleave(BS, 1), None, CONV["stride"],
                                                CONV["padding"], CONV["dilation"], 1)),
}
WRITES = {
    "first values": lambda a, b, sa, sb: a.neg_(),
    "second values": lambda a, b, sa, sb: b.neg_(),
    "first scale": lambda a, b, sa, sb: sa.mul_(2),
    "second scale": lambda a, b, sa, sb: sb.mul_(2),
}
# the second operand of matmul_mx is an activation; that of linear_mx / conv2d_mx is a weight (below).  conv2d_mx asks for the flag on
# the weight's scale too, linear_mx leaves the weight's scale to the packer's check.
STALE = [(op, write) for op in OPS for write in ("first values", "first scale")] + \
        [("matmul_mx", "second values"), ("matmul_mx", "second scale"), ("conv2d_mx", "second scale")]
WEIGHT = [("linear_mx", "second values"), ("linear_mx", "second scale"), ("conv2d_mx", "second values")]


def fresh(op):
    ax_a, ax_b = OPS[op][:2]
    a0, b0 = sources()[op]
    (a, sa), (b, sb) = quantized(a0, ax_a), quantized(b0, ax_b)
    return a, b, sa, sb


def untouched(op):
    from quantized_training import mx_gemm
    mx_gemm.STATS.reset()
    y = OPS[op][2](*fresh(op))
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0), f"{op}: the untouched call"
    return y


@pytest.mark.parametrize("op,write", STALE, ids=[f"{op}-{w.replace(' ', '_')}" for op, w in STALE])
def test_a_write_in_place_sends_the_call_to_the_composite(nv, op, write):
    from quantized_training import mx_gemm
    call, composite = OPS[op][2:]
    y0 = untouched(op)
    p = fresh(op)
    WRITES[write](*p)
    mx_gemm.STATS.reset()
    y = call(*p)
    stats = (mx_gemm.STATS.native, mx_gemm.STATS.fallback)
    want = composite(*p)
    assert y.shape == want.shape == y0.shape and y.dtype == want.dtype
    same, moved = torch.equal(bits_of(y), bits_of(want)), not torch.equal(bits_of(y), bits_of(y0))
    print(f"{op}, {write}: stats {stats}, equals the composite on the modified tensors {same}, differs from the untouched call {moved}")
    assert same, f"{op}, {write}: not the composite of the modified tensors"
    assert moved, f"{op}, {write}: the untouched call's result"
    assert stats == (0, 1), f"{op}, {write}"


@pytest.mark.parametrize("op,write", WEIGHT, ids=[f"{op}-{w.replace(' ', '_')}" for op, w in WEIGHT])
def test_a_written_to_weight_is_packed_again(nv, op, write):
    """The cache key of the constant operand carries the version counters: the call stays native and multiplies the new values, the
    same bits as for a weight (and scale) that held them from the start."""
    from quantized_training import mx_gemm
    call = OPS[op][2]
    y0 = untouched(op)
    a, b, sa, sb = fresh(op)
    call(a, b, sa, sb)                                              # the weight's operand is cached now
    WRITES[write](a, b, sa, sb)
    mx_gemm.STATS.reset()
    y = call(a, b, sa, sb)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0), f"{op}, {write}"
    a2, b2, sa2, sb2 = fresh(op)
    if write == "second values":
        b2 = -b2
    else:
        sb2 = sb2 * 2
    want = call(a2, b2, sa2, sb2)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (2, 0), f"{op}, {write}: the weight that held the values from the start"
    assert torch.equal(bits_of(y), bits_of(want)) and not torch.equal(bits_of(y), bits_of(y0)), f"{op}, {write}"


def test_inference_mode_keeps_the_native_route(nv):
    from quantized_training import mx_gemm
    x0, w0 = sources()["linear_mx"]
    w, sw = quantized(w0, -1)
    x, sx = quantized(x0, -1)
    mx_gemm.STATS.reset()
    y0 = torch.ops.quantized_ops.linear_mx(x, w, None, input_scale=sx, weight_scale=sw, block_size=BS)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0)
    with torch.inference_mode():
        x, sx = quantized(x0, -1)
        assert x.is_inference()
        y = torch.ops.quantized_ops.linear_mx(x, w, None, input_scale=sx, weight_scale=sw, block_size=BS)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (2, 0)
    assert torch.equal(bits_of(y), bits_of(y0))
