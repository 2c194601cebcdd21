"""conv2d_mx for integer and codebook operands: qt_conv2d_mxi (csrc/qt_mxi_conv.hip) through the C ABI and through the operator (mx_conv.py).
    y[n, ho, wo, co] = rd( bias[co] + sum_{(r, s, kb)} (sx[n, hi, wi, kb] sw[co, r, s, kb]) p ),   p = sum_{c in block kb} x[n, hi, wi, c] w[co, r, s, c]
The reference is that sum in fp64 over taps and blocks, by torch slicing of the zero-padded NHWC operands.  Data, exact tier and the derived
bound are test_gpu_mx_int_gemm.py's with nblk = kh kw Cin / bs.  Counting: a call that the float or the integer family looked at as its own
and neither took is one fallback; fp16 and QT_MX_GEMM=0 are looked at by neither and count nothing, as test_gpu_conv_mx.py pins."""
import pytest
import torch
import torch.nn.functional as F

from kernel_launch import Guarded, nv, stream  # noqa: F401
from quantized_training import mx_conv
from test_gpu_mx_int_gemm import (BF16, DTYPES, F32, bits, bound_of, captured, exact_problem, lookup64, ptr, quantized, reset, stats,
                                  tolerance_problem)

pytestmark = pytest.mark.gpu
PAD = 4096


def shapes(bs):
    """(N, Cin, H, W, Cout, (kh, kw), stride, padding, dilation)"""
    return {"one tile": (1, bs, 5, 5, 16, (1, 1), (1, 1), (0, 0), (1, 1)), "3x3 ragged": (3, bs, 9, 7, 136, (3, 3), (1, 1), (1, 1), (1, 1)),
            "asymmetric": (2, 2 * bs, 11, 9, 72, (3, 2), (2, 1), (1, 0), (1, 2)), "strided 1x1": (2, 256, 6, 6, 40, (1, 1), (2, 2), (0, 0), (1, 1)),
            "5x5": (1, bs, 12, 12, 24, (5, 5), (1, 1), (2, 2), (1, 1))}


def conv_terms(x, sx, w, sw, bs, shape):
    """(y64, S) [N, Ho, Wo, Cout]: the fp64 sum of the terms p sx sw over taps and blocks, and the sum of their magnitudes.  x [N, H, W, Cin]
    and w [Cout, kh, kw, Cin] hold integers, sx / sw their block scales along the last axis."""
    _, cin, h, wd, cout, (kh, kw), (sh, sw_), (ph, pw), (dh, dw) = shape
    ho, wo = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (wd + 2 * pw - dw * (kw - 1) - 1) // sw_ + 1
    xp, sp = (F.pad(t.double(), (0, 0, pw, pw, ph, ph)) for t in (x, sx))
    y = torch.zeros(x.shape[0], ho, wo, cout, dtype=torch.float64, device=x.device)
    S = torch.zeros_like(y)
    for r in range(kh):
        for s in range(kw):
            rows, cols = slice(r * dh, r * dh + (ho - 1) * sh + 1, sh), slice(s * dw, s * dw + (wo - 1) * sw_ + 1, sw_)
            for kb in range(cin // bs):
                p = xp[:, rows, cols, kb * bs:(kb + 1) * bs] @ w[:, r, s, kb * bs:(kb + 1) * bs].double().t()
                t = p * sp[:, rows, cols, kb, None] * sw[:, r, s, kb].double()
                y += t
                S += t.abs()
    return y, S


def as_conv(problem, shape):                                        # the GEMM test's a [1, M, K], b [1, N, K], bias [N] as x, w and bias [Cout]
    n, cin, h, wd, cout, (kh, kw), _, _, _ = shape
    a, sa, b, sb, bias = problem[:5]
    return a.view(n, h, wd, cin), sa.view(n, h, wd, -1), b.view(cout, kh, kw, cin), sb.view(cout, kh, kw, -1), bias[:cout].contiguous()


def run_conv(nv, x, sx, w, sw, bs, dtype, bias, shape, y):
    n, cin, h, wd, cout, (kh, kw), (sh, sw_), (ph, pw), (dh, dw) = shape
    rc = nv.lib().qt_conv2d_mxi(x.data_ptr(), sx.data_ptr(), w.data_ptr(), sw.data_ptr(), bs, y, int(dtype == F32), ptr(bias), n, h, wd, cin, cout,
                                kh, kw, sh, sw_, ph, pw, dh, dw, stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", sorted(shapes(32)))
@pytest.mark.parametrize("bs", [32, 64, 128])
def test_exact_tier_is_the_fp64_sum_rounded_once(nv, bs, name):
    """Operands between margins of 0xFF codes / NaN scales, the output between guard bands; two launches give the same bits."""
    shape = shapes(bs)[name]
    n, cin, h, wd, cout, (kh, kw), _, _, _ = shape
    x, sx, w, sw, bias = as_conv(exact_problem(n * h * wd, cout * kh * kw, cin, bs, 1, seed=bs + len(name)), shape)
    y64, S = conv_terms(x, sx, w, sw, bs, shape)
    assert float((S + bias.abs().double()).max()) < 2.0 ** 24 * 0.25, "the data do not keep every partial sum an fp32 number"
    raws = [torch.full((t.numel() + 2 * PAD,), f, dtype=t.dtype, device="cuda") for t, f in ((x, -1), (sx, float("nan")), (w, -1), (sw, float("nan")))]
    for raw, t in zip(raws, (x, sx, w, sw)):
        raw[PAD:PAD + t.numel()] = t.reshape(-1)
    views, before = [r[PAD:-PAD] for r in raws], [r.clone() for r in raws]
    for dtype, np_dtype in ((BF16, "uint16"), (F32, "float32")):
        for bv in (None, bias.to(dtype)):
            want = bits((y64 + (bv.double() if bv is not None else 0.0)).to(F32).to(dtype)).cpu()
            runs = []
            for _ in range(2):
                out = Guarded(tuple(y64.shape), np_dtype)
                assert run_conv(nv, *views, bs, dtype, bv, shape, out.ptr) == 0 and out.intact()
                runs.append(torch.from_numpy(out.host().view("int16" if dtype == BF16 else "int32")))
            assert torch.equal(runs[0], want), f"bs {bs}, {name}, {dtype}, bias {bv is not None}: {int((runs[0] != want).sum())} of {want.numel()} differ"
            assert torch.equal(runs[0], runs[1]), "two launches differ"
    assert all(torch.equal(r.view(torch.uint8), r0.view(torch.uint8)) for r, r0 in zip(raws, before)), "an operand or its margin was written"


@pytest.mark.parametrize("kind", ["fp8_e5m3", "amax"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", [32, 64, 128])
def test_tolerance_tier_against_fp64_and_the_composite(nv, bs, dtype, kind):
    """|y - y64| <= u_out |y64| + (nblk + 3) 2^-24 S; in bf16 the native error must not exceed that of the composite on the same operands."""
    shape = shapes(bs)["3x3 ragged"]
    n, cin, h, wd, cout, (kh, kw), stride, padding, dilation = shape
    x, sx, w, sw, bias = as_conv(tolerance_problem(n * h * wd, cout * kh * kw, cin, bs, dtype, kind, seed=bs + len(kind)), shape)
    y64, S = conv_terms(x, sx, w, sw, bs, shape)
    y64, S = y64 + bias.double(), S + bias.abs().double()
    got = torch.full(y64.shape, float("nan"), dtype=dtype, device="cuda")
    rc = run_conv(nv, x, sx.float(), w, sw.float(), bs, dtype, bias, shape, got.data_ptr())
    err, bound = (got.double() - y64).abs(), bound_of(y64, S, kh * kw * cin // bs, dtype)
    print(f"\n[conv2d_mxi bs {bs} {dtype} {kind}] largest error {float(err.max()):.3e}, largest error / bound {float((err / bound).max()):.3f}")
    assert rc == 0 and bool((err <= bound).all()), f"{int((err > bound).sum())} elements outside the bound, worst ratio {float((err / bound).max())}"
    if dtype == BF16:
        dx, dw_ = ((t.to(dtype) * s.repeat_interleave(bs, -1)).permute(0, 3, 1, 2) for t, s in ((x, sx), (w, sw)))
        cerr = (F.conv2d(dx, dw_, bias, stride, padding, dilation).permute(0, 2, 3, 1).double() - y64).abs()
        assert float(err.max()) <= float(cerr.max()), f"the composite's largest error is {float(cerr.max()):.3e}"


REFUSALS = [(f"NULL {p}", {p: None}, "BAD_ARG") for p in ("x", "sx", "w", "sw", "y")] + [(f"{k} = {v}", {k: v}, "BAD_ARG") for k, v in (
    ("N", -1), ("H", 0), ("Cout", -1), ("kh", 0), ("sh", 0), ("dw", 0), ("ph", -1), ("Cin", 0), ("bs", 16), ("bs", 96), ("Cin", 96), ("Cin", 32),
    ("pw", 2 ** 20), ("sh", 2 ** 20))] + [
    ("block size 256", dict(bs=256, Cin=256), "BAD_ARG"), ("N Ho Wo = 2^31", dict(N=2 ** 11, H=2 ** 10, W=2 ** 10, kh=1, kw=1, ph=0, pw=0), "BAD_ARG"),
    ("kh kw Cin = 2^31", dict(H=2 ** 12, W=2 ** 12, Cin=2 ** 11, kh=2 ** 10, kw=2 ** 10, ph=0, pw=0), "BAD_ARG"),
    ("x codes = 2^31 bytes", dict(H=2 ** 13, W=2 ** 12, sh=2 ** 6, sw_=2 ** 6, kh=1, kw=1, ph=0, pw=0), "BAD_ARG"),
    ("w codes = 2^31 bytes", dict(Cout=2 ** 21, Cin=1024, kh=1, kw=1, ph=0, pw=0), "BAD_ARG"),
    ("kh dh = 2^20", dict(H=2 ** 21, W=1, kh=2, kw=1, dh=2 ** 19, ph=0, pw=0), "BAD_ARG"),
    ("x codes off 16 bytes", dict(x=8), "UNALIGNED"), ("w codes off 16 bytes", dict(w=4), "UNALIGNED"), ("x scales off 4 bytes", dict(sx=2), "UNALIGNED"),
    ("w scales off 4 bytes", dict(sw=1), "UNALIGNED"), ("bf16 y off 2 bytes", dict(y=1), "UNALIGNED"), ("fp32 y off 4 bytes", dict(y=2, f32=1), "UNALIGNED"),
    ("bf16 bias off 2 bytes", dict(bias=1), "UNALIGNED"), ("fp32 bias off 4 bytes", dict(bias=2, f32=1), "UNALIGNED")]


@pytest.mark.parametrize("kw,code", [pytest.param(kw, code, id=label) for label, kw, code in REFUSALS])
def test_refusals_before_the_first_hip_call(nv, kw, code):
    """Each rule returns its code and leaves the output untouched (pointers: an offset in bytes from a valid address, or NULL)."""
    buf = {k: torch.zeros(8192, dtype=torch.uint8, device="cuda") for k in ("x", "sx", "w", "sw", "bias")}
    out = Guarded((8192,), "uint8")
    a = dict(bs=64, f32=0, N=1, H=5, W=5, Cin=64, Cout=16, kh=3, kw=3, sh=1, sw_=1, ph=1, pw=1, dh=1, dw=1, y=out.ptr, **{k: v.data_ptr() for k, v in buf.items()})
    for k, v in kw.items():
        a[k] = (a[k] + v if v is not None else None) if k in buf or k == "y" else v
    rc = nv.lib().qt_conv2d_mxi(*(a[k] for k in ("x", "sx", "w", "sw", "bs", "y", "f32", "bias", "N", "H", "W", "Cin", "Cout", "kh", "kw", "sh", "sw_", "ph",
                                                   "pw", "dh", "dw")), stream())
    torch.cuda.synchronize()
    assert rc == getattr(nv, "QT_ERR_" + code) != 0 and out.untouched()


# ---- the operator ---------------------------------------------------------------------------------------------------------------------------
CONFIGS = {"int6_bs64_e5m3": ("int6", "int6", 64, "fp8_e5m3"), "int6_x_nf4_6": ("int6", "nf4_6", 64, "fp8_e5m3"), "int8_bs32": ("int8", "int8", 32, None)}
GEOM = ((2, 1), (1, 0), (1, 2))                                     # stride, padding, dilation


@pytest.fixture
def every_shape(monkeypatch):
    """The route rule is a statement about speed; these tests are about results."""
    monkeypatch.setattr(mx_conv, "_APPLY_INT_CONV_RULE", False)
    reset()


def operands(name, dtype, channels_last=False, cin=128, seed=21):
    fx, fw, bs, sf = CONFIGS[name]
    g = torch.Generator().manual_seed(seed)
    x0, w0 = (torch.randn(2, cin, 11, 9, generator=g) * 2).to(dtype).cuda(), (torch.randn(72, cin, 3, 2, generator=g) * 0.3).to(dtype).cuda()
    if channels_last:
        x0 = x0.contiguous(memory_format=torch.channels_last)
    (x, sx, xc), (w, sw, wc) = quantized(x0, fx, bs, 1, sf), quantized(w0, fw, bs, 1, sf)
    return dict(x=x, w=w, bias=torch.randn(72, generator=g).to(dtype).cuda(), sx=sx, sw=sw, bs=bs, xc=xc, wc=wc, groups=1)


def conv_mx(p):
    return torch.ops.quantized_ops.conv2d_mx(p["x"], p["w"], p["bias"], *GEOM, p["groups"], input_scale=p["sx"], weight_scale=p["sw"],
                                             block_size=p["bs"], input_code=p["xc"], weight_code=p["wc"])


def composite(p):
    """decomposed.py's composite restated: codebook lookup, scales repeated over their blocks, F.conv2d."""
    dx, dw_ = ((c[t.to(torch.long)].to(t.dtype) if c is not None else t) * s.repeat_interleave(p["bs"], 1)[:, :t.shape[1]]
               for t, s, c in ((p["x"], p["sx"], p["xc"]), (p["w"], p["sw"], p["wc"])))
    return F.conv2d(dx, dw_, p["bias"], *GEOM, p["groups"])


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_conv2d_mx_takes_the_integer_route(nv, every_shape, name, dtype, channels_last):
    p = operands(name, dtype, channels_last)
    y = conv_mx(p)
    assert stats() == (1, 0) and y.dtype == dtype and y.shape == (2, 72, 6, 7) and y.permute(0, 2, 3, 1).is_contiguous()
    x, sx, w, sw = (t.permute(0, 2, 3, 1) for t in (lookup64(p["x"], p["xc"]), p["sx"], lookup64(p["w"], p["wc"]), p["sw"]))
    y64, S = conv_terms(x, sx, w, sw, p["bs"], (2, 128, 11, 9, 72, (3, 2)) + GEOM)
    y64, S = y64 + p["bias"].double(), S + p["bias"].abs().double()
    err, bound = (y.permute(0, 2, 3, 1).double() - y64).abs(), bound_of(y64, S, 6 * 128 // p["bs"], dtype)
    assert bool((err <= bound).all()), float((err / bound).max())


DECLINES = [("groups = 2", lambda p, mp: p.update(groups=2, w=p["w"][:, :64].contiguous(), sw=p["sw"][:, :1].contiguous()), (0, 1)),
            ("Cin % bs != 0", lambda p, mp: p.update(operands("int6_bs64_e5m3", BF16, cin=96)), (0, 1)),
            ("a float input with an integer weight",
             lambda p, mp: p.update(zip(("x", "sx"), quantized(torch.randn(2, 128, 11, 9, device="cuda").to(BF16), "fp8_e4m3", 64, 1, pow2=True))), (0, 1)),
            ("a class the route rule does not list",
             lambda p, mp: (mp.setattr(mx_conv, "_APPLY_INT_CONV_RULE", True), mp.setattr(mx_conv, "_int_conv_route_takes", lambda *a: False)), (0, 1)),
            ("fp16", lambda p, mp: p.update({k: p[k].half() for k in ("x", "w", "sx", "sw", "bias")}), (0, 0)),
            ("QT_MX_GEMM=0", lambda p, mp: mp.setenv("QT_MX_GEMM", "0"), (0, 0))]


@pytest.mark.parametrize("change,count", [pytest.param(c, n, id=label) for label, c, n in DECLINES])
def test_declines_run_the_composite(nv, every_shape, change, count, monkeypatch):
    """(under the library's deterministic algorithms: its default choice for the fp16 problem gives other bits from call to call)"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    p = operands("int6_bs64_e5m3", BF16)
    conv_mx(p)
    assert stats() == (1, 0), "the untouched call"
    change(p, monkeypatch)
    reset()
    y, want = conv_mx(p), composite(p)
    assert stats() == count
    assert y.dtype == want.dtype and y.shape == want.shape and torch.equal(y.view(torch.int16), want.view(torch.int16))


def test_weight_rewrite_graph_replay_and_the_float_route(nv, every_shape, monkeypatch):
    p, q = operands("int6_x_nf4_6", BF16), operands("int6_x_nf4_6", BF16)
    y0 = conv_mx(p)                                                 # the weight's operand is cached now
    p["w"].copy_(15 - p["w"])
    q["w"] = 15 - q["w"]
    y, want = conv_mx(p), conv_mx(q)
    assert stats() == (3, 0) and torch.equal(bits(y), bits(want)) and not torch.equal(bits(y), bits(y0))

    def acts(k):                                                    # the pack and the kernel are captured; replays run on other activations
        x0 = (torch.randn(2, 128, 11, 9, generator=torch.Generator().manual_seed(k)) * k).to(BF16).cuda()
        return list(quantized(x0, "int6", 64, 1, "fp8_e5m3")[:2])
    captured(lambda x, sx: conv_mx(dict(q, x=x, sx=sx)), acts(1), [acts(2), acts(3)])
    assert stats()[1] == 0 and stats()[0] >= 6
    # a float-format problem still takes qt_conv2d_mx
    calls = []
    for name in ("qt_conv2d_mx", "qt_conv2d_mxi"):
        monkeypatch.setattr(nv.lib(), name, lambda *a, _n=name, _r=getattr(nv.lib(), name): (calls.append(_n), _r(*a))[1])
    (x, sx, _), (w, sw, _) = (quantized(torch.randn(*s, device="cuda").to(BF16), "fp8_e4m3", 32, 1, pow2=True) for s in ((2, 64, 9, 7), (24, 64, 3, 3)))
    reset()
    torch.ops.quantized_ops.conv2d_mx(x, w, None, [1, 1], [1, 1], [1, 1], 1, input_scale=sx, weight_scale=sw, block_size=32)
    assert stats() == (1, 0) and calls == ["qt_conv2d_mx"]
