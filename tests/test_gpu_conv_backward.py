"""The backward products of a QAT convolution on the device: qt_conv2d_dgrad_bf16 / qt_conv2d_wgrad_bf16 (csrc/qt_conv_backward.hip)
through the C ABI against the fp64 gradients, their plan, determinism (split-K, graph replay), guard regions and declines, and the
autograd routing of conv_route._Conv2dInTree under QT_CONV_GEMM."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, G)
import gen_golden_conv as gc  # noqa: E402

import quantized_training as qt  # noqa: E402
from quantized_training import _native, conv_route, fused  # noqa: E402
from quantized_training.modules import qat as nnqat  # noqa: E402
from quantized_training.qconfig import get_qconfig  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _leave_no_routes():
    from quantized_training import optim
    from quantized_training.modules.qat.linear import GEMM_ROUTES
    tables = (conv_route.CONV_ROUTES, GEMM_ROUTES, fused.ROUTES, fused.LT_ALGOS, optim.ROUTES)
    before = [dict(t) for t in tables]
    yield
    for t, b in zip(tables, before):
        t.clear()
        t.update(b)


def _make_args(**kw):
    a = qt.add_qspec_args().parse_args([])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


IMPL = gc.Impl(nnqat, get_qconfig, qt.quantize, _make_args)

# (N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, dh, dw): the forward's EXACT_GRID (tests/test_gpu_conv.py) ...
FORWARD_GRID = [
    (2, 15, 13, 64, 72, 3, 3, 1, 1, 1, 1, 1, 1),          # 3 x 3, H W = 195: no tile height divides it; Cout ragged against the k tile
    (1, 15, 13, 128, 200, 1, 1, 1, 1, 0, 0, 1, 1),        # 1 x 1, one image, Cout 200
    (3, 15, 13, 64, 64, 5, 5, 2, 2, 2, 2, 1, 1),          # 5 x 5, stride 2, padding 2
    (2, 15, 13, 64, 72, 3, 5, 1, 2, 1, 2, 1, 1),          # non-square filter, mixed stride and padding
    (2, 15, 13, 256, 64, 3, 3, 1, 1, 2, 2, 2, 2),         # dilation 2
    (2, 15, 13, 64, 72, 3, 3, 2, 2, 0, 0, 1, 1),          # stride 2, no padding
    (1, 7, 7, 512, 8, 1, 1, 1, 1, 0, 0, 1, 1),            # Cin 512, the narrowest Cout: ONE k tile of 8 live channels
    (1, 9, 9, 64, 16, 1, 1, 1, 1, 0, 0, 1, 1),            # ONE k tile: zero tiles fill the ring
    (16, 48, 48, 64, 200, 3, 3, 1, 1, 1, 1, 1, 1),        # many images
    (8, 56, 56, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1),          # dgrad 128 x 64 tiles; wgrad 9 tiles: the deepest split
]
# ... and what the backward adds
EXTRA = [
    (2, 9, 11, 64, 64, 1, 1, 2, 2, 0, 0, 1, 1),           # 1 x 1 stride 2: three input pixels in four are reached by no tap
    (2, 16, 14, 64, 64, 3, 3, 2, 2, 0, 0, 1, 1),          # 3 x 3 stride 2 no padding on 16 x 14: the last row and column lie under no window
    (2, 9, 9, 64, 40, 3, 3, 1, 1, 1, 1, 1, 1),            # Cout 40: ragged against the k tile (dgrad declines it, wgrad takes it)
    (16, 48, 48, 128, 64, 1, 1, 1, 1, 0, 0, 1, 1),        # dgrad 128 x 128 tiles
    (1, 6, 6, 512, 512, 3, 3, 1, 1, 1, 1, 1, 1),          # wgrad 128 x 128 tiles, one k tile; dgrad K = 4608
    (4, 17, 19, 512, 512, 2, 4, 1, 1, 0, 0, 1, 1),        # wgrad 128 x 128 tiles with two splits
]
EXACT_GRID = FORWARD_GRID + EXTRA
# the input gradient takes whole k tiles of 64 output channels only: the forward grid's ragged geometries once more with such a Cout
DGRAD_EXTRA = [
    (2, 15, 13, 64, 128, 3, 5, 1, 2, 1, 2, 1, 1),         # non-square filter, mixed stride and padding, two k tiles per tap
    (2, 15, 13, 64, 64, 3, 3, 2, 2, 0, 0, 1, 1),          # stride 2, no padding, odd plane
    (2, 15, 13, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1),          # 3 x 3, H W = 195: no tile height divides it
    (1, 9, 9, 64, 64, 1, 1, 1, 1, 0, 0, 1, 1),            # ONE k tile: zero tiles fill the ring
    (1, 15, 13, 128, 192, 1, 1, 1, 1, 0, 0, 1, 1),        # 1 x 1, one image, three k tiles
]
_ids = lambda c: "x".join(str(v) for v in c)  # noqa: E731


def _out_hw(c):
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw = c
    return (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plan(c):
    d, g = _native.QtConv2dProductPlan(), _native.QtConv2dProductPlan()
    rc = _native.lib().qt_conv2d_backward_plan(*c, ctypes.byref(d), ctypes.byref(g))
    return rc, d, g


def _dgrad(gy, w, gx, c):
    _native.note_device(0)
    return _native.lib().qt_conv2d_dgrad_bf16(gy.data_ptr(), w.data_ptr(), gx.data_ptr(), *c, _stream())


def _scratch(c):
    """(workspace, tickets) of the plan's size -- (None, None) without a split."""
    rc, _, g = _plan(c)
    assert rc == 0
    if g.ksplit <= 1:
        return None, None
    return (torch.empty((g.ws_bytes // 4,), dtype=torch.float32, device=DEV), torch.zeros((g.n_tickets,), dtype=torch.int32, device=DEV))


def _wgrad(gy, x, gw, c, ws, tickets):
    _native.note_device(0)
    return _native.lib().qt_conv2d_wgrad_bf16(gy.data_ptr(), x.data_ptr(), gw.data_ptr(), *c, ws.data_ptr() if ws is not None else None,
                                              ws.numel() * 4 if ws is not None else 0, tickets.data_ptr() if tickets is not None else None,
                                              tickets.numel() if tickets is not None else 0, _stream())


def _dgrad_fp64(gy, w, c):
    """The input gradient in double, tap by tap (a double GEMM per tap): gy NHWC, w [Cout][kh][kw][Cin] -> [N, H, W, Cin]."""
    n, h, wd, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw = c
    ho, wo = _out_hw(c)
    gp = torch.zeros((n, h + 2 * ph, wd + 2 * pw, cin), dtype=torch.float64, device=gy.device)
    g2 = gy.double().reshape(-1, cout)
    for r in range(kh):
        for s in range(kw):
            gp[:, r * dh: r * dh + sh * (ho - 1) + 1: sh, s * dw: s * dw + sw * (wo - 1) + 1: sw, :] += g2.matmul(w[:, r, s, :].double()).view(n, ho, wo, cin)
    return gp[:, ph: ph + h, pw: pw + wd, :].contiguous()


def _wgrad_fp64(gy, x, c):
    """The weight gradient in double, tap by tap: gy, x NHWC -> [Cout][kh][kw][Cin]."""
    n, h, wd, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw = c
    ho, wo = _out_hw(c)
    xp = F.pad(x.double(), (0, 0, pw, pw, ph, ph))
    g2t = gy.double().reshape(-1, cout).t()
    out = torch.zeros((cout, kh, kw, cin), dtype=torch.float64, device=gy.device)
    for r in range(kh):
        for s in range(kw):
            patch = xp[:, r * dh: r * dh + sh * (ho - 1) + 1: sh, s * dw: s * dw + sw * (wo - 1) + 1: sw, :]
            out[:, r, s, :] = g2t.matmul(patch.reshape(-1, cin))
    return out


def _amax(k):
    return int(min(127, np.sqrt((2 ** 24 - 2 ** 14) / k)))


def _exact(shape, amax, exp, g):
    return (torch.randint(-amax, amax + 1, shape, generator=g).float() * 2.0 ** exp).bfloat16().to(DEV)


def _exact_operands(c, seed, product):
    """int8 codes times powers of two on both operands of `product`, the code range sized by its contraction length K so that every sum
    is an integer below 2^24 in its unit: exact in fp32 whatever the order of the additions.  -> (gy, w, x), NHWC / [Cout][kh][kw][Cin]."""
    n, h, wd, cin, cout, kh, kw = c[:7]
    ho, wo = _out_hw(c)
    amax = _amax(kh * kw * cout if product == "dgrad" else n * ho * wo)
    g = torch.Generator(device="cpu").manual_seed(seed)
    gy = _exact((n, ho, wo, cout), amax, -4, g)
    w = _exact((cout, kh, kw, cin), amax, -7, g)
    x = _exact((n, h, wd, cin), amax, -5, g)
    return gy, w, x


def _bits(t):
    return t.contiguous().view(torch.int16)


def _nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)


# ---- 1. exact tier through the C ABI -------------------------------------------------------------------------------------------------
def test_code_range_of_the_existing_grid():
    for c in FORWARD_GRID:
        ho, wo = _out_hw(c)
        assert _amax(c[5] * c[6] * c[4]) >= 21 and _amax(c[0] * ho * wo) >= 21


@pytest.mark.parametrize("case", EXACT_GRID + DGRAD_EXTRA, ids=_ids)
def test_dgrad_kernel_exact(case):
    gy, w, _ = _exact_operands(case, 41, "dgrad")
    n, h, wd, cin = case[:4]
    gx = _nan((n, h, wd, cin))                                          # every element must be written
    if case[4] % 64 != 0:                                               # Cout ragged against the k tile: declined, nothing launched
        rc, d, g = _plan(case)
        assert rc == 0 and d.taken == 0 and g.taken == 1
        assert _dgrad(gy, w, gx, case) == _native.QT_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert torch.isnan(gx.float()).all()
        return
    assert _dgrad(gy, w, gx, case) == 0
    ref = _dgrad_fp64(gy, w, case).float().bfloat16()                  # exact in fp32: ONE rounding
    assert torch.equal(_bits(gx), _bits(ref))
    gx2 = _nan((n, h, wd, cin))
    assert _dgrad(gy, w, gx2, case) == 0 and torch.equal(_bits(gx), _bits(gx2))


@pytest.mark.parametrize("case", EXACT_GRID, ids=_ids)
def test_wgrad_kernel_exact(case):
    gy, _, x = _exact_operands(case, 43, "wgrad")
    cin, cout, kh, kw = case[3:7]
    ws, tickets = _scratch(case)
    gw = _nan((cout, kh, kw, cin))
    assert _wgrad(gy, x, gw, case, ws, tickets) == 0
    ref = _wgrad_fp64(gy, x, case).float().bfloat16()
    assert torch.equal(_bits(gw), _bits(ref))
    gw2 = _nan((cout, kh, kw, cin))
    assert _wgrad(gy, x, gw2, case, ws, tickets) == 0 and torch.equal(_bits(gw), _bits(gw2))
    if tickets is not None:
        assert int(tickets.abs().sum().item()) == 0


def test_unreached_input_pixels_are_written_zero():
    for c in (EXTRA[0], EXTRA[1]):
        gy, w, _ = _exact_operands(c, 47, "dgrad")
        gx = _nan((c[0], c[1], c[2], c[3]))
        assert _dgrad(gy, w, gx, c) == 0
        assert torch.isfinite(gx.float()).all()
    # 1 x 1 stride 2: odd rows and columns are reached by no tap; 16 x 14 under 3 x 3 stride 2: the last row and column
    assert (gx[:, 15, :, :] == 0).all() and (gx[:, :, 13, :] == 0).all() and (gx[:, :15, :13, :] != 0).any()


# ---- 2. plan coverage ----------------------------------------------------------------------------------------------------------------
def test_backward_plan_reaches_every_instantiation():
    seen_d, seen_w, splits = set(), set(), set()
    for c in EXACT_GRID + DGRAD_EXTRA:
        rc, d, g = _plan(c)
        n, h, wd, cin, cout, kh, kw = c[:7]
        assert rc == 0 and d.taken == (cout % 64 == 0) and g.taken == 1
        ho, wo = _out_hw(c)
        if d.taken:
            assert d.tiles_m == -(-n * h * wd // d.tile_m) and d.tiles_n == -(-cin // d.tile_n) and d.k_tiles == kh * kw * (cout // 64)
            assert d.ksplit == 1 and d.ws_bytes == 0 and d.n_tickets == 0
            seen_d.add((d.tile_m, d.tile_n))
        assert g.tiles_m == -(-cout // g.tile_m) and g.tiles_n == -(-kh * kw * cin // g.tile_n) and g.k_tiles == -(-n * ho * wo // 64)
        assert 1 <= g.ksplit <= 32 and g.ksplit <= g.k_tiles
        if g.ksplit > 1:
            assert g.ws_bytes == g.tiles_m * g.tiles_n * g.ksplit * g.tile_m * g.tile_n * 4 and g.n_tickets == g.tiles_m * g.tiles_n
        else:
            assert g.ws_bytes == 0 and g.n_tickets == 0
        seen_w.add((g.tile_m, g.tile_n, g.ksplit > 1))
        splits.add(g.ksplit)
    assert seen_d == {(128, 128), (128, 64), (64, 64)}, seen_d          # every instantiation of the dgrad launcher
    assert seen_w == {(128, 128, False), (128, 128, True), (64, 64, False), (64, 64, True)}, seen_w   # of the wgrad launcher, both endings
    assert 1 in splits and max(splits) > 1, splits


# ---- 3. tolerance tier on random operands --------------------------------------------------------------------------------------------
TOL_CASES = [
    (32, 56, 56, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1),          # wgrad K = 100 352
    (32, 7, 7, 512, 512, 3, 3, 1, 1, 1, 1, 1, 1),          # dgrad K = 4608
    (32, 28, 28, 256, 512, 1, 1, 2, 2, 0, 0, 1, 1),        # a stride-2 1 x 1 downsample
    (32, 14, 14, 256, 256, 3, 3, 1, 1, 1, 1, 1, 1),
]


@pytest.mark.parametrize("case", TOL_CASES, ids=_ids)
def test_backward_kernels_random_operands(case):
    """|g - ref| <= 2^-8 |ref| + 2^-18 conv(|a|, |b|) against the fp64 gradients computed on the device (the bound of
    test_gpu_parity.test_train_gemm_against_fp64_products and of the forward's tolerance tier: the fp32 error and the magnitude term both
    grow linearly with the contraction length)."""
    n, h, wd, cin, cout, kh, kw = case[:7]
    ho, wo = _out_hw(case)
    g = torch.Generator(device=DEV).manual_seed(5)
    gy = (torch.randn((n, ho, wo, cout), generator=g, device=DEV) * 0.1).bfloat16()
    w = (torch.randn((cout, kh, kw, cin), generator=g, device=DEV) * 0.05).bfloat16()
    x = torch.randn((n, h, wd, cin), generator=g, device=DEV).bfloat16()
    gx = _nan((n, h, wd, cin))
    assert _dgrad(gy, w, gx, case) == 0
    ref, mag = _dgrad_fp64(gy, w, case), _dgrad_fp64(gy.abs(), w.abs(), case)
    worst_d = ((gx.double() - ref).abs() / (2.0 ** -8 * ref.abs() + 2.0 ** -18 * mag).clamp_min(1e-300)).max().item()
    del ref, mag
    ws, tickets = _scratch(case)
    gw = _nan((cout, kh, kw, cin))
    assert _wgrad(gy, x, gw, case, ws, tickets) == 0
    ref, mag = _wgrad_fp64(gy, x, case), _wgrad_fp64(gy.abs(), x.abs(), case)
    worst_w = ((gw.double() - ref).abs() / (2.0 ** -8 * ref.abs() + 2.0 ** -18 * mag).clamp_min(1e-300)).max().item()
    print(f"{case}: worst err / bound: dgrad {worst_d:.3f}, wgrad {worst_w:.3f}")
    assert worst_d <= 1.0, worst_d
    assert worst_w <= 1.0, worst_w


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------
def test_determinism_split_k_and_graph_replay():
    case = FORWARD_GRID[9]
    rc, d, gp = _plan(case)
    assert rc == 0 and gp.ksplit > 1
    n, h, wd, cin, cout, kh, kw = case[:7]
    ho, wo = _out_hw(case)
    g = torch.Generator(device=DEV).manual_seed(9)
    gy = (torch.randn((n, ho, wo, cout), generator=g, device=DEV) * 0.1).bfloat16()
    w = (torch.randn((cout, kh, kw, cin), generator=g, device=DEV) * 0.05).bfloat16()
    x = torch.randn((n, h, wd, cin), generator=g, device=DEV).bfloat16()
    ws, tickets = _scratch(case)
    outs = []
    for _ in range(2):
        gx, gw = _nan((n, h, wd, cin)), _nan((cout, kh, kw, cin))
        assert _dgrad(gy, w, gx, case) == 0 and _wgrad(gy, x, gw, case, ws, tickets) == 0
        outs.append((gx, gw))
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert int(tickets.abs().sum().item()) == 0
    ggx, ggw = _nan((n, h, wd, cin)), _nan((cout, kh, kw, cin))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # a single-branch graph
        assert _dgrad(gy, w, ggx, case) == 0 and _wgrad(gy, x, ggw, case, ws, tickets) == 0
    ggx.fill_(float("nan"))
    ggw.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(ggx), _bits(outs[0][0])) and torch.equal(_bits(ggw), _bits(outs[0][1]))
    assert int(tickets.abs().sum().item()) == 0


# ---- 5. guards -----------------------------------------------------------------------------------------------------------------------
def _guarded(t, guard=1 << 16):
    """A copy of `t` between two NaN-filled guard regions -> (whole buffer, view, guard)."""
    buf = torch.full((t.numel() + 2 * guard,), float("nan"), dtype=torch.bfloat16, device=DEV)
    view = buf[guard: guard + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view, guard


def _guards_intact(buf, numel, guard):
    return bool(torch.isnan(buf[:guard].float()).all() and torch.isnan(buf[guard + numel:].float()).all())


@pytest.mark.parametrize("case", [FORWARD_GRID[0], DGRAD_EXTRA[2], FORWARD_GRID[2], FORWARD_GRID[4], EXTRA[2]],
                         ids=["3x3p1cout72", "3x3p1", "5x5s2p2", "3x3d2p2", "cout40"])
def test_guard_regions_padding_and_ragged_rows(case):
    n, h, wd, cin, cout, kh, kw = case[:7]
    ho, wo = _out_hw(case)
    assert (n * h * wd) % 64 != 0 and (n * ho * wo) % 64 != 0           # ragged row tiles resp. a ragged last k tile
    # dgrad: NaN around gy, w and gx; gx itself pre-filled with NaN
    gy, w, _ = _exact_operands(case, 51, "dgrad")
    bgy, vgy, gd = _guarded(gy)
    bw, vw, _ = _guarded(w)
    bgx, vgx, _ = _guarded(_nan((n, h, wd, cin)))
    if cout % 64 == 0:
        assert _dgrad(vgy, vw, vgx, case) == 0
        assert torch.isfinite(vgx.float()).all()
        assert torch.equal(_bits(vgx), _bits(_dgrad_fp64(gy, w, case).float().bfloat16()))
    else:                                                               # declined: gx is left as it was
        assert _dgrad(vgy, vw, vgx, case) == _native.QT_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert torch.isnan(vgx.float()).all()
    assert _guards_intact(bgy, gy.numel(), gd) and _guards_intact(bw, w.numel(), gd) and _guards_intact(bgx, vgx.numel(), gd)
    # wgrad: NaN around gy, x and gw
    gy, _, x = _exact_operands(case, 53, "wgrad")
    bgy, vgy, _ = _guarded(gy)
    bx, vx, _ = _guarded(x)
    bgw, vgw, _ = _guarded(_nan((cout, kh, kw, cin)))
    ws, tickets = _scratch(case)
    assert _wgrad(vgy, vx, vgw, case, ws, tickets) == 0
    assert torch.isfinite(vgw.float()).all()
    assert torch.equal(_bits(vgw), _bits(_wgrad_fp64(gy, x, case).float().bfloat16()))
    assert _guards_intact(bgy, gy.numel(), gd) and _guards_intact(bx, x.numel(), gd) and _guards_intact(bgw, vgw.numel(), gd)


# ---- 6. declines ---------------------------------------------------------------------------------------------------------------------
def test_declines():
    from quantized_training._native import QT_ERR_BAD_ARG, QT_ERR_UNALIGNED
    ok = (8, 56, 56, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1)
    rc, _, gp = _plan(ok)
    assert rc == 0 and gp.ksplit > 1
    gy, w, x = _exact_operands(ok, 3, "wgrad")
    gx, gw = _nan(tuple(x.shape)), _nan(tuple(w.shape))
    ws, tickets = _scratch(ok)
    stem = (8, 56, 56, 3, 64, 3, 3, 1, 1, 1, 1, 1, 1)
    odd = (8, 56, 56, 64, 12, 3, 3, 1, 1, 1, 1, 1, 1)
    for bad in (stem, odd):
        rc, d, g = _plan(bad)
        assert rc == QT_ERR_BAD_ARG and d.taken == 0 and g.taken == 0
        assert _dgrad(gy, w, gx, bad) == QT_ERR_BAD_ARG
        assert _wgrad(gy, x, gw, bad, ws, tickets) == QT_ERR_BAD_ARG

    def off(t):
        return torch.empty(t.numel() + 8, dtype=torch.bfloat16, device=DEV)[1: 1 + t.numel()].view(t.shape)

    assert _dgrad(off(gy), w, gx, ok) == QT_ERR_UNALIGNED and _dgrad(gy, off(w), gx, ok) == QT_ERR_UNALIGNED
    assert _dgrad(gy, w, off(gx), ok) == QT_ERR_UNALIGNED
    assert _wgrad(off(gy), x, gw, ok, ws, tickets) == QT_ERR_UNALIGNED and _wgrad(gy, off(x), gw, ok, ws, tickets) == QT_ERR_UNALIGNED
    assert _wgrad(gy, x, gw, ok, ws[: ws.numel() // 2], tickets) == QT_ERR_BAD_ARG       # a workspace too small
    assert _wgrad(gy, x, gw, ok, ws, tickets[: gp.n_tickets - 1]) == QT_ERR_BAD_ARG    # too few tickets
    assert _wgrad(gy, x, gw, ok, None, tickets) == QT_ERR_BAD_ARG                      # a null workspace with split > 1
    assert _wgrad(gy, x, gw, ok, ws, None) == QT_ERR_BAD_ARG
    ragged = (8, 56, 56, 64, 72, 3, 3, 1, 1, 1, 1, 1, 1)                               # Cout % 64 != 0: the input gradient alone declines
    rc, d, g = _plan(ragged)
    assert rc == 0 and d.taken == 0 and g.taken == 1
    assert _dgrad(gy, w, gx, ragged) == QT_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(gx.float()).all() and torch.isnan(gw.float()).all()             # nothing was launched
    assert int(tickets.abs().sum().item()) == 0


# ---- 7. autograd ---------------------------------------------------------------------------------------------------------------------
def _bwd_routes():
    return {k: v for k, v in fused.routes_report().items() if k.startswith("conv2d_dgrad ") or k.startswith("conv2d_wgrad ")}


def _exact_gy(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randint(-31, 32, shape, generator=g).float() * 2.0 ** -4).bfloat16().to(DEV)


def _twin_grads(monkeypatch, mode, build, x0, gy, prepare=None):
    monkeypatch.setenv("QT_CONV_GEMM", mode)
    conv_route.CONV_ROUTES.clear()
    m = build()
    if prepare is not None:
        prepare(m)
    x = x0.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    y = m(x)
    y.backward(gy)
    grads = {"gx": x.grad, "gw": m.weight.grad}
    if m.bias is not None:
        grads["gb"] = m.bias.grad
    return grads, dict(conv_route.CONV_ROUTES)


def _twin_bwd_routes(routes):
    return sorted((k.split(" ")[0], v) for k, v in routes.items() if not k.startswith("conv2d "))


def _expected_bwd_routes(cout):
    """Under QT_CONV_GEMM=1: the weight gradient in-tree; the input gradient too where Cout is whole k tiles of 64 channels (the twins of
    the fixtures have 16 and 8 output channels: theirs stays with the library; the Cout = 64 problems below send it in-tree)."""
    return [("conv2d_dgrad", "in_tree_bf16_conv" if cout % 64 == 0 else "library_conv"), ("conv2d_wgrad", "in_tree_bf16_conv")]


def test_conv2d_twin_gradients_equal_the_library(monkeypatch):
    kw, shape = gc.LAYERS["conv2d"][1], gc.LAYERS["conv2d"][2]
    g = torch.Generator(device="cpu").manual_seed(61)
    x0 = _exact(shape, 127, -5, g).contiguous(memory_format=torch.channels_last)
    gy = _exact_gy((shape[0], kw["out_channels"], shape[2], shape[3]), 63).contiguous(memory_format=torch.channels_last)
    build = lambda: gc.build_layer(IMPL, "int8_pow2", "conv2d", DEV)   # noqa: E731
    ours, routes = _twin_grads(monkeypatch, "1", build, x0, gy)
    assert _twin_bwd_routes(routes) == _expected_bwd_routes(kw["out_channels"]), routes
    lib, routes0 = _twin_grads(monkeypatch, "0", build, x0, gy)
    assert set(routes0.values()) == {"library_conv"} and all(k.startswith("conv2d ") for k in routes0), routes0
    for name in ours:
        assert ours[name].shape == lib[name].shape and torch.equal(ours[name], lib[name]), name
    assert ours["gx"].is_contiguous(memory_format=torch.channels_last)


def test_convbn2d_twin_gradients_equal_the_library(monkeypatch):
    g = torch.Generator(device="cpu").manual_seed(67)
    x0 = _exact(gc.CONVBN_INPUT, 127, -5, g).contiguous(memory_format=torch.channels_last)
    gy = _exact_gy((gc.CONVBN_INPUT[0], gc.CONVBN["out_channels"], gc.CONVBN_INPUT[2], gc.CONVBN_INPUT[3]), 69)

    def prepare(m):
        # BN factors that are powers of two: the gradient that reaches the convolution stays on its power-of-two grid
        with torch.no_grad():
            m.bn.weight.fill_(0.5)
            m.bn.running_var.fill_(1.0)
            m.bn.running_mean.zero_()

    build = lambda: gc.build_convbn(IMPL, "int8_pow2", "train_frozen", DEV)   # noqa: E731
    ours, routes = _twin_grads(monkeypatch, "1", build, x0, gy, prepare)
    assert _twin_bwd_routes(routes) == _expected_bwd_routes(gc.CONVBN["out_channels"]), routes
    lib, routes0 = _twin_grads(monkeypatch, "0", build, x0, gy, prepare)
    assert set(routes0.values()) == {"library_conv"}, routes0
    for name in ours:
        assert ours[name].shape == lib[name].shape and torch.equal(ours[name], lib[name]), name


def _route_call(x, w, b):
    return conv_route.conv2d_or_none(x, w, b, (1, 1), (1, 1), (1, 1), 1)


@pytest.mark.parametrize("cout", [64, 72])
def test_routes_under_the_switch_and_needs_input_grad_subsets(monkeypatch, cout):
    case = (4, 14, 14, 64, cout, 3, 3, 1, 1, 1, 1, 1, 1)
    gy_e, w_e, x_e = _exact_operands(case, 71, "wgrad")
    x0, w0 = x_e.permute(0, 3, 1, 2), w_e.permute(0, 3, 1, 2).contiguous()
    b0 = _exact_gy((cout,), 73)
    gy = gy_e.permute(0, 3, 1, 2)

    def run(mode, rx, rw, rb):
        monkeypatch.setenv("QT_CONV_GEMM", mode)
        conv_route.CONV_ROUTES.clear()
        x, w, b = x0.detach().clone(memory_format=torch.preserve_format).requires_grad_(rx), w0.detach().clone().requires_grad_(rw), b0.detach().clone().requires_grad_(rb)
        y = _route_call(x, w, b)
        if y is None:
            assert mode == "0"
            y = F.conv2d(x, w, b, 1, 1, 1, 1)
        y.backward(gy)
        return (x.grad, w.grad, b.grad), _bwd_routes()

    full, routes = run("1", True, True, True)
    lib, routes0 = run("0", True, True, True)
    assert routes0 == {}, routes0                                       # "0": nothing of the backward is in-tree
    for a, b in zip(full, lib):
        assert torch.equal(a, b)
    if cout % 64 != 0:
        # Cout ragged against the k tile: the input gradient stays with the library, the weight gradient goes in-tree
        assert sorted((k.split(" ")[0], v) for k, v in routes.items()) == [("conv2d_dgrad", "library_conv"), ("conv2d_wgrad", "in_tree_bf16_conv")]
        return
    assert len(routes) == 2 and set(routes.values()) == {"in_tree_bf16_conv"}, routes
    # a frozen weight: only the input gradient is computed and recorded
    launched = []
    real_d, real_w = conv_route._launch_dgrad, conv_route._launch_wgrad
    monkeypatch.setattr(conv_route, "_launch_dgrad", lambda *a: launched.append("dgrad") or real_d(*a))
    monkeypatch.setattr(conv_route, "_launch_wgrad", lambda *a: launched.append("wgrad") or real_w(*a))
    (gx, gw, gb), routes = run("1", True, False, False)
    assert gw is None and gb is None and torch.equal(gx, full[0]) and launched == ["dgrad"], launched
    assert [k.split(" ")[0] for k in routes] == ["conv2d_dgrad"]
    # an input without grad: only the weight and bias gradients
    del launched[:]
    (gx, gw, gb), routes = run("1", False, True, True)
    assert gx is None and torch.equal(gw, full[1]) and torch.equal(gb, full[2]) and launched == ["wgrad"], launched
    assert [k.split(" ")[0] for k in routes] == ["conv2d_wgrad"]
    # under "1" with every product in-tree the library is not called
    called = []
    real = conv_route._library_backward

    monkeypatch.setattr(conv_route, "_library_backward", lambda *a: called.append(1) or real(*a))
    run("1", True, True, True)
    assert called == []


def test_nchw_and_channels_last_gradients_agree(monkeypatch):
    monkeypatch.setenv("QT_CONV_GEMM", "1")
    case = (4, 14, 14, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1)
    g = torch.Generator(device=DEV).manual_seed(79)
    x0 = torch.randn((4, 64, 14, 14), generator=g, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    w0 = (torch.randn((64, 64, 3, 3), generator=g, device=DEV) * 0.05).bfloat16()
    gy_cl = torch.randn((4, 64, 14, 14), generator=g, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    gy_nchw = gy_cl.contiguous()
    assert gy_nchw.is_contiguous() and not gy_nchw.is_contiguous(memory_format=torch.channels_last)
    outs = []
    for gy in (gy_cl, gy_nchw):
        # x and w are copies of leaves: a hook on them sees the gradients as the Function returns them (a leaf's .grad is laid out like
        # the leaf, whatever layout autograd was handed)
        xl, wl = x0.detach().clone(memory_format=torch.preserve_format).requires_grad_(), w0.detach().clone().requires_grad_()
        x, w = xl.clone(memory_format=torch.preserve_format), wl.clone()
        got = {}
        x.register_hook(lambda t: got.__setitem__("gx", t))
        w.register_hook(lambda t: got.__setitem__("gw", t))
        _route_call(x, w, None).backward(gy)
        assert torch.equal(xl.grad, got["gx"]) and torch.equal(wl.grad, got["gw"])
        outs.append((got["gx"], got["gw"]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][0].is_contiguous(memory_format=torch.channels_last) and outs[0][1].shape == w0.shape
    assert outs[0][1].permute(0, 2, 3, 1).is_contiguous()               # [Cout][kh][kw][Cin] memory under the weight's logical shape
    assert case[4] == w0.shape[0]


def test_mini_cnn_trains_bit_reproducibly(monkeypatch):
    monkeypatch.setenv("QT_CONV_GEMM", "1")
    runs = []
    for _ in range(2):
        conv_route.CONV_ROUTES.clear()
        m = gc.train_cnn(gc.build_cnn(IMPL, DEV))
        runs.append({k: v.detach().clone() for k, v in m.state_dict().items()})
        n = gc.CNN_INPUT[0]
        routes = _bwd_routes()
        assert routes[f"conv2d_dgrad {n}×64×12×10 → 64 k3x3 s2x2 p0x0 d1x1"] == "in_tree_bf16_conv", routes
        assert routes[f"conv2d_wgrad {n}×64×12×10 → 64 k3x3 s2x2 p0x0 d1x1"] == "in_tree_bf16_conv", routes
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert all(torch.isfinite(v.float()).all() for k, v in runs[0].items() if v.is_floating_point())
