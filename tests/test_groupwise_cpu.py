"""Group-wise affine (qs=group_wise_affine) without a GPU: the ctypes table against the header, the routing predicates of the
fused kernels, and the extracted torch composite against the oracle bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import qt_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = [f"qt_{fam}_{io}" for fam in ("fake_quant_gwa", "quantize_blocks", "dequantize_blocks") for io in ("bf16", "f32")]
RANGES = [(0, 15), (-8, 7), (0, 3), (0, 255)]
SHAPES = [((8, 512), -1, 32), ((8, 512), -1, 128), ((6, 256), -1, 256), ((2, 3, 128, 64), -1, 16), ((2, 3, 128, 64), -2, 64),
          ((4, 256, 40), -2, 64)]


def recipe(shape, seed):
    """A seeded normal draw times a per-row magnitude 10**U(-3, 2); then, on the flattened tensor, zero and constant blocks,
    a negative stretch, +Inf, -Inf, NaN and a value whose distance to the block minimum overflows."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 2, shape[:-1] + (1,))).astype(np.float32)
    f = x.reshape(-1)
    f[0:256] = 0.0
    f[256:512] = 1.5
    f[512:768] = -np.abs(f[512:768])
    f[800], f[1100], f[1400] = np.inf, -np.inf, np.nan
    f[-1] = 3.0e38
    return x


def test_native_table_binds_the_six_entry_points_with_the_headers_argument_counts():
    from quantized_training import _native
    header = open(os.path.join(ROOT, "include", "qt_hip.h")).read()
    for name in ENTRY_POINTS:
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", header, re.S)
        assert m, f"{name} is not declared in include/qt_hip.h"
        res, args = _native.SIGNATURES[name]
        assert res is _native.c_int
        assert len(args) == len(m.group(1).split(",")), name
    assert _native.ABI_VERSION == 3 and re.search(r"#define\s+QT_ABI_VERSION\s+3\b", header)


def test_fake_quant_routing_predicate():
    from quantized_training.fake_quantize import gwa_block_view as view
    bf, f32 = torch.bfloat16, torch.float32
    # taken: last axis and strided, int or one-element sequence, negative or not
    assert view((8, 512), bf, 128, -1) == (8, 512, 1)
    assert view((8, 512), bf, 32, (1,)) == (8, 512, 1)
    assert view((8, 512), f32, 4, [-1]) == (8, 512, 1)
    assert view((2, 3, 128, 64), bf, 64, -2) == (6, 128, 64)
    assert view((2, 3, 128, 64), f32, 1, 2) == (6, 128, 64)
    assert view((4, 256, 40), bf, 64, -2) == (4, 256, 40)
    assert view((4, 256, 36), f32, 64, 1) == (4, 256, 36)
    assert view((4, 96, 8), bf, 48, 1) == (4, 96, 8)                     # strided blocks need not be a power of two
    assert view((512,), bf, 512, 0) == (1, 512, 1)
    assert view((16, 64, 1), bf, 16, 1) == (16, 64, 1)                   # a trailing axis of one is the last-axis layout
    # declined
    assert view((8, 100), bf, 32, -1) is None                            # padding: the axis is no multiple of the block
    assert view((4, 64, 20), bf, 32, -2) is None                         # inner % 8
    assert view((4, 64, 20), f32, 32, -2) == (4, 64, 20)                 # ... but a multiple of 4 fp32 elements
    assert view((4, 64, 18), f32, 32, -2) is None
    assert view((8, 512), bf, (1, 32), (0, 1)) is None                   # tuple block size
    assert view((8, 512), bf, 32, (0, 1)) is None                        # several block axes
    assert view((8, 512), torch.float16, 32, -1) is None
    assert view((8, 512), bf, 4, -1) is None                             # below one 16-byte vector of bf16
    assert view((8, 512), f32, 512, -1) is None                          # above 64 lanes of fp32
    assert view((8, 96), bf, 48, -1) is None                             # last-axis blocks are powers of two
    assert view((2, 1024, 8), bf, 1024, 1) is None                       # strided blocks stop at 512 rows
    assert view((0, 512), bf, 32, -1) is None
    assert view((8, 512), bf, 32, 2) is None
    assert view((8, 512), bf, 32.0, -1) is None


def test_quantize_dequantize_routing_predicate():
    from quantized_training.decomposed import block_param_view as view
    bf = torch.bfloat16
    assert view((64, 256), (64, 8), 32, bf) == (64, 256, 1)
    assert view((2, 3, 128, 64), (2, 3, 2, 64), 64, bf) == (6, 128, 64)
    assert view((64, 256), (64, 256), 1, bf) is None                      # no dimension differs
    assert view((64, 256), (2, 8), 32, bf) is None                        # two dimensions differ
    assert view((64, 256), (64, 4), 32, bf) is None                       # not by the block size
    assert view((64, 256), (8,), 32, bf) is None                          # parameters of lower rank
    assert view((64, 256), (64, 8), 32, torch.float16) is None


@pytest.mark.parametrize("io", ["bf16", "f32"])
@pytest.mark.parametrize("shape,ax,bs", SHAPES, ids=[f"{'x'.join(map(str, s))}-ax{a}-bs{b}" for s, a, b in SHAPES])
def test_extracted_composite_equals_the_oracle(shape, ax, bs, io):
    from quantized_training.fake_quantize import group_wise_affine_composite
    bf16 = io == "bf16"
    x = recipe(shape, seed=bs + len(shape))
    if bf16:
        bits = o.f32_to_bf16(x).reshape(shape)
        x = o.bf16_to_f32(bits).reshape(shape)
        xt = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)
    else:
        xt = torch.from_numpy(x)

    def canon(t):
        t = t.contiguous()
        if bf16:
            return o.canon_nan16(t.view(torch.int16).numpy().view(np.uint16))
        return o.canon_nan32(t.view(torch.int32).numpy().view(np.uint32))

    def canon_ref(a):
        a = np.ascontiguousarray(a, np.float32)
        return o.canon_nan16(o.f32_to_bf16(a).reshape(a.shape)) if bf16 else o.canon_nan32(a.view(np.uint32))

    for qmin, qmax in RANGES:
        scale, zp = torch.empty(0, dtype=xt.dtype), torch.empty(0, dtype=xt.dtype)
        y = group_wise_affine_composite(xt, scale, zp, ax, bs, qmin, qmax)
        ey, es, ez = o.group_wise_affine_fake_quant(x, bf16, ax, bs, qmin, qmax)
        assert tuple(scale.shape) == es.shape and tuple(zp.shape) == ez.shape
        assert np.array_equal(canon(y), canon_ref(ey)), (qmin, qmax)
        assert np.array_equal(canon(scale), canon_ref(es)), (qmin, qmax)
        assert np.array_equal(canon(zp), canon_ref(ez)), (qmin, qmax)
