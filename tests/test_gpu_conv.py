"""QAT convolutions on the device: qt_conv2d_bf16 (csrc/qt_conv.hip) through the C ABI against the fp64 convolution, its padding and
ragged-tile behaviour, what it declines, and the Conv2d / ConvBn2d twins, their autograd wiring and the mini CNN through the route."""
import ctypes
import json
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
    """routes_report() of later tests lists what THEY ran: the process-wide route tables (the convolutions' and, for the mini CNN's
    Linear and its SGD steps, the training GEMMs' and the optimizer's) are put back as this test found them."""
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

# (N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, dh, dw, bias)
EXACT_GRID = [
    (2, 15, 13, 64, 72, 3, 3, 1, 1, 1, 1, 1, 1, True),        # 3 x 3, H W = 195: no tile height divides it; Cout ragged against 64
    (1, 15, 13, 128, 200, 1, 1, 1, 1, 0, 0, 1, 1, False),     # 1 x 1, one image, Cout 200
    (3, 15, 13, 64, 64, 5, 5, 2, 2, 2, 2, 1, 1, True),        # 5 x 5, stride 2, padding 2
    (2, 15, 13, 64, 72, 3, 5, 1, 2, 1, 2, 1, 1, False),       # non-square filter, mixed stride and padding
    (2, 15, 13, 256, 64, 3, 3, 1, 1, 2, 2, 2, 2, True),       # dilation 2
    (2, 15, 13, 64, 72, 3, 3, 2, 2, 0, 0, 1, 1, True),        # stride 2, no padding
    (1, 7, 7, 512, 8, 1, 1, 1, 1, 0, 0, 1, 1, True),          # Cin 512, the narrowest Cout
    (1, 9, 9, 64, 16, 1, 1, 1, 1, 0, 0, 1, 1, False),         # ONE k tile: zero tiles fill the ring
    (16, 48, 48, 64, 200, 3, 3, 1, 1, 1, 1, 1, 1, True),      # many images: 128 x 128 tiles, Cout ragged against 128
    (8, 56, 56, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1, False),       # 128 x 64 tiles
]


def _out_hw(c):
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, _ = c
    return (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def _capi(x, w, bias, y, c):
    """qt_conv2d_bf16 on raw NHWC / [Cout][kh][kw][Cin] buffers; returns the status."""
    n, h, wd, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, _ = c
    _native.note_device(0)
    return _native.lib().qt_conv2d_bf16(x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(), n, h, wd, cin,
                                        cout, kh, kw, sh, sw, ph, pw, dh, dw, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _conv_fp64(x, w, bias, c):
    """The convolution in double, tap by tap (a double GEMM per tap): x NHWC, w [Cout][kh][kw][Cin] -> [N, Ho, Wo, Cout]."""
    n, h, wd, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, _ = c
    ho, wo = _out_hw(c)
    xp = F.pad(x.double(), (0, 0, pw, pw, ph, ph))
    out = torch.zeros((n, ho, wo, cout), dtype=torch.float64, device=x.device)
    for r in range(kh):
        for s in range(kw):
            patch = xp[:, r * dh: r * dh + sh * (ho - 1) + 1: sh, s * dw: s * dw + sw * (wo - 1) + 1: sw, :]
            out += patch.reshape(-1, cin).matmul(w[:, r, s, :].double().t()).view(n, ho, wo, cout)
    return out if bias is None else out + bias.double()


def _exact_operands(c, seed):
    """int8 codes times powers of two on both operands, sized so that every dot product (+ bias) is an integer below 2^24 in units of
    2^-12: exact in fp32 whatever the order of the additions."""
    n, h, wd, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, has_bias = c
    k = kh * kw * cin
    amax = int(min(127, np.sqrt((2 ** 24 - 2 ** 14) / k)))
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randint(-amax, amax + 1, (n, h, wd, cin), generator=g).float() * 2.0 ** -5).bfloat16().to(DEV)
    w = (torch.randint(-amax, amax + 1, (cout, kh, kw, cin), generator=g).float() * 2.0 ** -7).bfloat16().to(DEV)
    b = (torch.randint(-127, 128, (cout,), generator=g).float() * 2.0 ** -6).bfloat16().to(DEV) if has_bias else None
    return x, w, b


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- 6. exact tier through the C ABI -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT_GRID, ids=lambda c: "x".join(str(v) for v in c[:-1]) + ("b" if c[-1] else ""))
def test_conv2d_kernel_exact(case):
    x, w, b = _exact_operands(case, 17)
    ho, wo = _out_hw(case)
    y = torch.empty((case[0], ho, wo, case[4]), dtype=torch.bfloat16, device=DEV)
    assert _capi(x, w, b, y, case) == 0
    ref = _conv_fp64(x, w, b, case).float().bfloat16()               # exact in fp32: ONE rounding
    assert torch.equal(_bits(y), _bits(ref))
    y2 = torch.empty_like(y)
    assert _capi(x, w, b, y2, case) == 0 and torch.equal(_bits(y), _bits(y2))


def _plan(c):
    out = [ctypes.c_int(0) for _ in range(5)]
    rc = _native.lib().qt_conv2d_plan(*c[:13], *[ctypes.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


def test_plan_reaches_every_tile_shape():
    seen = set()
    for c in EXACT_GRID:
        rc, (bm, bn, tm, tn, kt) = _plan(c)
        assert rc == 0
        ho, wo = _out_hw(c)
        assert tm == -(-c[0] * ho * wo // bm) and tn == -(-c[4] // bn) and kt == c[5] * c[6] * c[3] // 64
        seen.add((bm, bn))
    assert seen == {(128, 128), (128, 64), (64, 64)}, seen            # every instantiation of the launcher


# ---- 7. tolerance tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [
    (32, 56, 56, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1, True),
    (32, 7, 7, 512, 512, 3, 3, 1, 1, 1, 1, 1, 1, False),             # K 4608
    (32, 7, 7, 2048, 512, 1, 1, 1, 1, 0, 0, 1, 1, True),             # K 2048, 1 x 1
    (32, 56, 56, 64, 256, 1, 1, 1, 1, 0, 0, 1, 1, False),
], ids=["56x56x64_3x3", "7x7x512_3x3", "7x7x2048_1x1", "56x56x64_1x1_256"])
def test_conv2d_kernel_random_operands(case):
    """|y - ref| <= 2^-8 |ref| + 2^-18 conv(|x|, |w|) against the fp64 convolution computed on the device (the bound of
    test_gpu_parity.test_train_gemm_against_fp64_products)."""
    n, h, wd, cin, cout, kh, kw = case[:7]
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((n, h, wd, cin), generator=g, device=DEV).bfloat16()
    w = (torch.randn((cout, kh, kw, cin), generator=g, device=DEV) * 0.05).bfloat16()
    b = torch.randn((cout,), generator=g, device=DEV).bfloat16() if case[-1] else None
    ho, wo = _out_hw(case)
    y = torch.empty((n, ho, wo, cout), dtype=torch.bfloat16, device=DEV)
    assert _capi(x, w, b, y, case) == 0
    ref = _conv_fp64(x, w, b, case)
    mag = _conv_fp64(x.abs(), w.abs(), None if b is None else b.abs(), case)
    worst = ((y.double() - ref).abs() / (2.0 ** -8 * ref.abs() + 2.0 ** -18 * mag).clamp_min(1e-300)).max().item()
    print(f"{case}: worst err / bound = {worst:.3f}")
    assert worst <= 1.0, worst


# ---- 8. padding reads zeros; rows past M are not stored -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [EXACT_GRID[0], EXACT_GRID[2], EXACT_GRID[4]], ids=["3x3p1", "5x5s2p2", "3x3d2p2"])
def test_padding_reads_zeros_and_ragged_rows_are_not_stored(case):
    x, w, b = _exact_operands(case, 23)
    guard = 1 << 16
    buf = torch.full((x.numel() + 2 * guard,), float("nan"), dtype=torch.bfloat16, device=DEV)
    xin = buf[guard: guard + x.numel()].view(x.shape)
    xin.copy_(x)
    ho, wo = _out_hw(case)
    m = case[0] * ho * wo
    assert m % 64 != 0
    ybuf = torch.full((m * case[4] + guard,), float("nan"), dtype=torch.bfloat16, device=DEV)
    y = ybuf[: m * case[4]].view(case[0], ho, wo, case[4])
    assert _capi(xin, w, b, y, case) == 0
    assert torch.isfinite(y.float()).all()
    assert torch.equal(_bits(y), _bits(_conv_fp64(x, w, b, case).float().bfloat16()))
    assert torch.isnan(ybuf[m * case[4]:].float()).all()
    assert torch.isnan(buf[:guard].float()).all() and torch.isnan(buf[guard + x.numel():].float()).all()


# ---- 9. declines ---------------------------------------------------------------------------------------------------------------------
def test_declines():
    from quantized_training._native import QT_ERR_BAD_ARG, QT_ERR_UNALIGNED
    ok = (2, 8, 8, 64, 16, 3, 3, 1, 1, 1, 1, 1, 1, False)
    x, w, _ = _exact_operands(ok, 3)
    y = torch.full((2, 8, 8, 16), float("nan"), dtype=torch.bfloat16, device=DEV)
    stem = (2, 8, 8, 3, 16, 3, 3, 1, 1, 1, 1, 1, 1, False)
    assert _capi(x, w, None, y, stem) == QT_ERR_BAD_ARG and _plan(stem)[0] == QT_ERR_BAD_ARG
    odd = (2, 8, 8, 64, 12, 3, 3, 1, 1, 1, 1, 1, 1, False)
    assert _capi(x, w, None, y, odd) == QT_ERR_BAD_ARG
    xoff = torch.empty(x.numel() + 8, dtype=torch.bfloat16, device=DEV)[1: 1 + x.numel()].view(x.shape)
    assert _capi(xoff, w, None, y, ok) == QT_ERR_UNALIGNED
    torch.cuda.synchronize()
    assert torch.isnan(y.float()).all()                                # nothing was launched


def test_module_declines_keep_the_library(monkeypatch):
    monkeypatch.setenv("QT_CONV_GEMM", "1")
    conv_route.CONV_ROUTES.clear()
    qc = gc.qconfig_of(IMPL, "e4m3")
    cases = {
        "grouped": (nn.Conv2d(64, 64, 3, padding=1, groups=4), torch.bfloat16),
        "stem": (nn.Conv2d(3, 64, 3, padding=1), torch.bfloat16),
        "fp32": (nn.Conv2d(64, 64, 3, padding=1), torch.float32),
    }
    for name, (flt, dtype) in cases.items():
        flt = gc.seed_params_(flt, 5).to(dtype).to(DEV)
        flt.qconfig = qc
        m = nnqat.Conv2d.from_float(flt).to(DEV)
        x = gc.rand_bf16(8, (2, flt.in_channels, 8, 8)).to(dtype).to(DEV)
        taps = []
        h = m.weight_fake_quant.register_forward_hook(lambda mod, a, out: taps.append(out.detach()))
        with torch.no_grad():
            y = m(x)
            want = F.conv2d(x, taps[0], m.bias, m.stride, m.padding, m.dilation, m.groups)
        h.remove()
        assert torch.equal(y, want), name
    report = fused.routes_report()
    convs = {k: v for k, v in report.items() if k.startswith("conv2d ")}
    assert len(convs) == 3 and set(convs.values()) == {"library_conv"}, convs
    # a view at an odd offset is declined as well
    flt = gc.seed_params_(nn.Conv2d(64, 16, 1), 5).bfloat16().to(DEV)
    flt.qconfig = qc
    m = nnqat.Conv2d.from_float(flt).to(DEV)
    base = torch.zeros(2 * 5 * 5 * 64 + 8, dtype=torch.bfloat16, device=DEV)
    xo = base[1: 1 + 2 * 5 * 5 * 64].view(2, 5, 5, 64).permute(0, 3, 1, 2)
    with torch.no_grad():
        m(xo)
    assert fused.routes_report()["conv2d 2×64×5×5 → 16 k1x1 s1x1 p0x0 d1x1"] == "library_conv"


# ---- 10. the twins on the device ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traces():
    npz = np.load(os.path.join(G, "conv_traces.npz"))
    with open(os.path.join(G, "conv_traces.json")) as f:
        return npz, json.load(f)


def _get(npz, key, dtype):
    return gc.from_bits(npz[key.replace("/", "__")], getattr(torch, dtype))


def _run_twin(monkeypatch, mode_env, build, xs, load_bn):
    monkeypatch.setenv("QT_CONV_GEMM", mode_env)
    conv_route.CONV_ROUTES.clear()
    m = build()
    calls = gc.run_trace(m, xs, load_bn)
    return calls, dict(conv_route.CONV_ROUTES)


@pytest.mark.parametrize("layer", ["conv2d", "convbn2d/train_update", "convbn2d/train_frozen", "convbn2d/eval"])
def test_twins_in_tree_equal_library_and_fixture(monkeypatch, traces, layer):
    npz, meta = traces
    spec = "int8_pow2"
    key = f"{spec}/{layer}"
    dt = meta[key]["dtypes"]
    xkey = f"{spec}/{layer.split('/')[0]}"
    xs = [_get(npz, f"{xkey}/x{i}", "bfloat16").to(DEV).contiguous(memory_format=torch.channels_last) for i in range(gc.N_CALLS)]
    if layer == "conv2d":
        build = lambda: gc.build_layer(IMPL, spec, "conv2d", DEV)     # noqa: E731
    else:
        build = lambda: gc.build_convbn(IMPL, spec, layer.split("/")[1], DEV)   # noqa: E731

    def load_bn(i, mod):
        for b in gc.BN_BUFFERS:
            getattr(mod.bn, b).copy_(_get(npz, f"{key}/call{i}/bn_before.{b}", dt["bn_before." + b]))

    load = load_bn if layer.endswith("train_update") else None
    ours, routes = _run_twin(monkeypatch, "1", build, xs, load)
    assert set(routes.values()) == {"in_tree_bf16_conv"}, routes
    lib, routes0 = _run_twin(monkeypatch, "0", build, xs, load)
    assert set(routes0.values()) == {"library_conv"}, routes0
    for i, (a, b) in enumerate(zip(ours, lib)):
        for name in ("wq", "scale", "amax_history"):
            want = _get(npz, f"{key}/call{i}/{name}", dt[name])
            assert np.array_equal(gc.bits(a[name]), gc.bits(want)), (layer, i, name, "against the CPU fixture")
            assert np.array_equal(gc.bits(a[name]), gc.bits(b[name])), (layer, i, name)
        assert a["out"].is_contiguous(memory_format=torch.channels_last)
        if layer.endswith("train_update") and a["out"].stride() != b["out"].stride():
            # the library handed the BN another memory format: its training-mode reduction runs in another order
            torch.testing.assert_close(a["out"], b["out"])
        else:
            assert np.array_equal(gc.bits(a["out"]), gc.bits(b["out"])), (layer, i, "out")


def test_nchw_and_channels_last_inputs_agree(monkeypatch, traces):
    npz, _ = traces
    monkeypatch.setenv("QT_CONV_GEMM", "1")
    x = _get(npz, "int8_pow2/conv2d/x0", "bfloat16").to(DEV)
    assert x.is_contiguous()
    outs = []
    for xin in (x, x.contiguous(memory_format=torch.channels_last)):
        m = gc.build_layer(IMPL, "int8_pow2", "conv2d", DEV)
        with torch.no_grad():
            outs.append(m(xin))
    assert outs[0].shape == outs[1].shape and torch.equal(outs[0], outs[1])
    assert outs[0].is_contiguous(memory_format=torch.channels_last)


# ---- 11. autograd wiring -------------------------------------------------------------------------------------------------------------
def test_autograd_against_the_library(monkeypatch):
    case = (4, 14, 14, 64, 72, 3, 3, 1, 1, 1, 1, 1, 1, True)
    xe, we, be = _exact_operands(case, 31)
    x0 = xe.permute(0, 3, 1, 2)                                        # logical NCHW over NHWC memory
    w0 = we.permute(0, 3, 1, 2).contiguous()
    # the incoming gradient on a power-of-two grid as well: with 784 resp. 648 terms per sum every gradient element is an integer below
    # 2^24 in its unit, exact in fp32 in ANY order -- a library backward that accumulates through atomics (its weight gradient differed
    # between two runs by a relative L2 distance of 1.0e-5 on random gradients) has one possible result here
    g = torch.Generator(device="cpu").manual_seed(77)
    gy = (torch.randint(-31, 32, (4, 72, 14, 14), generator=g).float() * 2.0 ** -4).bfloat16().to(DEV).contiguous(memory_format=torch.channels_last)

    def grads(mode):
        monkeypatch.setenv("QT_CONV_GEMM", mode)
        x, w, b = x0.detach().clone(memory_format=torch.preserve_format).requires_grad_(), w0.detach().clone().requires_grad_(), be.detach().clone().requires_grad_()
        y = conv_route.conv2d_or_none(x, w, b, (1, 1), (1, 1), (1, 1), 1)
        assert (y is not None) == (mode == "1")
        if y is None:
            y = F.conv2d(x, w, b, 1, 1, 1, 1)
        y.backward(gy)
        return y.detach(), x.grad, w.grad, b.grad

    lib1, lib2, ours = grads("0"), grads("0"), grads("1")
    # (the forwards are not compared here: with a bias the library rounds the convolution to bf16 and adds the bias in a second
    # rounding, the kernel adds it in fp32 and rounds once -- items 6 and 10 pin the forward; the gradients do not depend on it)
    names = ("gx", "gw", "gb")
    deterministic = all(torch.equal(a, b) for a, b in zip(lib1[1:], lib2[1:]))

    def rel(a, b):
        return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()

    noise = {n: rel(a, b) for n, a, b in zip(names, lib1[1:], lib2[1:])}
    print(f"library backward deterministic: {deterministic}; relative L2 distance of its two runs: {noise}")
    for n, a, b in zip(names, ours[1:], lib1[1:]):
        assert a.shape == b.shape and a.dtype == b.dtype
        if deterministic:
            assert torch.equal(a, b), n
        else:
            assert rel(a, b) <= 2.0 * noise[n], (n, rel(a, b), noise[n])


# ---- 12. the mini CNN through quantize() ---------------------------------------------------------------------------------------------
def test_mini_cnn_trains_routes_and_replays(monkeypatch):
    monkeypatch.setenv("QT_CONV_GEMM", "1")
    conv_route.CONV_ROUTES.clear()
    m = gc.build_cnn(IMPL, DEV)
    gc.train_cnn(m)
    assert all(torch.isfinite(p).all() for p in m.parameters())
    convs = {k: v for k, v in fused.routes_report().items() if k.startswith("conv2d ")}
    n = gc.CNN_INPUT[0]
    assert convs[f"conv2d {n}×64×12×10 → 64 k3x3 s2x2 p0x0 d1x1"] == "in_tree_bf16_conv", convs
    assert convs[f"conv2d {n}×3×12×10 → 64 k3x3 s1x1 p1x1 d1x1"] == "library_conv", convs
    gc.freeze_for_eval(m)
    x = gc.rand_bf16(3400, gc.CNN_INPUT).to(DEV)
    with torch.no_grad():
        eager = m(x).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                  # a single-branch graph
            out = m(x)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
