"""qt_attention_fp8_gqa (csrc/qt_attention_fp8_gqa.hip), the streaming FP8 attention core on UNREPEATED K / V^T for grouped-query heads:
through the C ABI into guarded buffers against the interval oracle's "online" model on K / V repeated G times (v holds one key per column:
every output is one exact product), bit for bit against qt_attention_fp8_long on codes repeated on the device, and through the module route."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import attention_cases as ac
from oracle import qt_oracle as o

from kernel_launch import Guarded, dev, inside, launch, nv, refused, same, stream  # noqa: F401
from test_gpu_attention_cores import Inputs, _bhsd, _fp8_codes, _fp8_tables, _ptr
from test_gpu_attention_fp8_long import _steps

pytestmark = pytest.mark.gpu

# name: (B, H, Hkv, Sq, Sk, D, format, mask(rng) or None, live)
CASES = {
    "h4_kv2_d128_e4m3_sq65_sk128_nomask": (1, 4, 2, 65, 128, 128, "e4m3", None, False),
    "h4_kv1_d64_e5m2_sq33_sk256_bias": (1, 4, 1, 33, 256, 64, "e5m2", lambda r: ac.bias((1, 4, 33, 256), r), False),
    "h8_kv1_d128_e4m3_sq17_sk1152_ragged": (1, 8, 1, 17, 1152, 128, "e4m3", lambda r: ac.ragged(17, 1152, r), True),
    "h4_kv2_d64_e4m3_sq256_sk256_causal": (1, 4, 2, 256, 256, 64, "e4m3", lambda r: ac.causal(256, 256), True),
    "h2_kv1_d128_e5m2_sq1_sk1280_nomask": (1, 2, 1, 1, 1280, 128, "e5m2", None, False),
    "h8_kv2_d64_e5m2_sq65_sk1280_padding0": (2, 8, 2, 65, 1280, 64, "e5m2", lambda r: ac.padding([1280, 0], 1280), True),
    "h4_kv2_d128_e5m2_sq65_sk1280_max_last": (1, 4, 2, 65, 1280, 128, "e5m2", lambda r: _steps(65, 1280, True), False),
}


def make_case(name):
    """(the oracle's case on K / V repeated G times, the unrepeated k and one-key-per-column v)"""
    B, H, Hkv, Sq, Sk, D, fmt, mask, live = CASES[name]
    q, k, v, rng = ac._qkv(name, B, H, Sq, Sk, D)
    k, v_one = k[:, :Hkv], ac.one_key_per_column(v[:, :Hkv])      # (its key choice depends on the head: repeated afterwards, a group's heads agree)
    c = ac.Case(name, "fp8", q, np.repeat(k, H // Hkv, 1), np.repeat(v_one, H // Hkv, 1), None if mask is None else mask(rng), fmt=fmt, live=live)
    c.kernel = "online"
    return c, k, v_one


def _core(nv, entry, heads, c, x, q8, k8, vt8, fmt, out, out8, live=False, simple=0, flag=False):
    """One launch of qt_attention_fp8_gqa (heads = (H, Hkv)) or qt_attention_fp8_long (heads = (H,)): mask read, or (live) the row extents
    with the caller's verdict (simple) or the device's (flag)."""
    rl, ls = (x.rl, x.ls) if live else (None, (0, 0, 0))
    return getattr(nv.lib(), entry)(q8.data_ptr(), k8.data_ptr(), vt8.data_ptr(), 0 if c.fmt == "e4m3" else 1, _ptr(x.mask), *x.ms, rl, *ls, simple,
                                    x.irr if flag else None, out, out8, ctypes.byref(fmt) if out8 else None, c.B, *heads, c.Sq, c.Sk, c.D, c.scaling, stream())


@pytest.mark.parametrize("name", list(CASES))
def test_attention_fp8_gqa_every_variant(nv, name):
    """Inside the interval; the output modes and the mask forms bit-equal; bit-equal to qt_attention_fp8_long on repeated codes; guards
    intact (launch); one graph replay bit-equal."""
    c, k, v_one = make_case(name)
    Hkv, G = k.shape[1], c.H // k.shape[1]
    iv, ivq = c.intervals(), c.intervals(out_fq=True)
    share, nonzero = iv.out.decided_share(), float(((iv.out.lo & 0x7FFF) != 0).mean())
    print(f"\n[{name}] decided {share:.4f}, non-zero {nonzero:.3f}")
    assert share >= 0.99 and nonzero >= 0.15, "the case decides too little"
    x = Inputs(nv, c)
    fmt = nv.format_for(c.fmt)
    q8, k8, v_dev = dev(_fp8_codes(c.q, c.fmt)), dev(_fp8_codes(k, c.fmt)), dev(v_one)
    s = c.Sk * c.D
    vt8 = dev(launch(lambda g: nv.lib().qt_value_codes_t(v_dev.data_ptr(), g["vt8"].ptr, c.B, Hkv, c.Sk, c.D, Hkv * s, s, c.D, ctypes.byref(fmt), stream()),
                     {"vt8": ((c.B, Hkv, c.D, c.Sk), np.uint8)}, f"qt_value_codes_t {name}")["vt8"])
    shape = (c.B, c.Sq, c.H, c.D)

    def run(mode, what, entry="qt_attention_fp8_gqa", heads=(c.H, Hkv), kv=(k8, vt8), **kw):
        specs = {k_: (shape, t) for k_, t in (("out", np.uint16), ("out8", np.uint8)) if mode in (k_, "both")}
        return launch(lambda g: _core(nv, entry, heads, c, x, q8, *kv, fmt, g["out"].ptr if "out" in g else None, g["out8"].ptr if "out8" in g else None, **kw),
                      specs, what)

    what = f"qt_attention_fp8_gqa {name}"
    r0 = run("out", what)
    inside(iv.out, _bhsd(r0["out"]), what, "attention_fp8_gqa")
    rb = run("both", what + " out + out8")
    inside(ivq.out, _bhsd(rb["out"]), what + " out + out8", "attention_fp8_gqa")
    same(rb["out"], o.vmap_bf16(r0["out"], c.qmap()), what + ": out is the map of the plain result")
    same(_fp8_tables(c.fmt)[rb["out8"]], rb["out"], what + ": the codes decode to out")
    same(run("out8", what + " codes only")["out8"], rb["out8"], what + ": codes only / out + out8")
    if c.live:
        forms = [("row extents", dict(simple=0)), ("device flag", dict(flag=True))]
        if not x.irregular:
            forms.append(("mask_is_simple", dict(simple=1)))
        for tag, kw in forms:
            same(run("out", f"{what} {tag}", live=True, **kw)["out"], r0["out"], f"{what}: {tag} / mask read")
        same(run("out8", what + " device flag, codes only", live=True, flag=True)["out8"], rb["out8"], what + ": device flag, codes only")
    # the streaming core on the same q8 with k8 / vt8 repeated on the device, as _repeat_kv orders the heads
    rep = (k8.repeat_interleave(G, 1).contiguous(), vt8.repeat_interleave(G, 1).contiguous())
    rl = run("both", what + ": qt_attention_fp8_long on repeated codes", entry="qt_attention_fp8_long", heads=(c.H,), kv=rep, live=c.live, flag=c.live)
    same(rb["out"], rl["out"], what + ": out / qt_attention_fp8_long")
    same(rb["out8"], rl["out8"], what + ": out8 / qt_attention_fp8_long")
    g_out, side, graph = Guarded(shape, np.uint16), torch.cuda.Stream(), torch.cuda.CUDAGraph()       # one graph replay against the eager result
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        assert _core(nv, "qt_attention_fp8_gqa", (c.H, Hkv), c, x, q8, k8, vt8, fmt, g_out.ptr, None, live=c.live, flag=c.live) == 0
    graph.replay()
    torch.cuda.synchronize()
    assert g_out.intact()
    same(g_out.host(), r0["out"], what + ": graph replay / eager")


def test_attention_fp8_gqa_refusals(nv):
    """What the entry point does not take: an error status, nothing written."""
    fmt, big = nv.format_for("e4m3"), dev(np.zeros(8 * 1280 * 128, np.uint8))
    spec = {"out": ((1, 65, 8, 128), np.uint16), "out8": ((1, 65, 8, 128), np.uint8)}

    def call(g, B=1, H=4, Hkv=2, Sk=256, D=64, out_off=0, out8_off=0, none=False):
        out, out8 = (None, None) if none else (g["out"].ptr + out_off, g["out8"].ptr + out8_off)
        return nv.lib().qt_attention_fp8_gqa(big.data_ptr(), big.data_ptr(), big.data_ptr(), 0, None, 0, 0, 0, None, 0, 0, 0, 0, None, out, out8,
                                             ctypes.byref(fmt), B, H, Hkv, 65, Sk, D, D ** -0.5, stream())

    for what, kw in (("Hkv = H", dict(Hkv=4)), ("H = 6, Hkv = 2", dict(H=6)), ("H % Hkv != 0", dict(Hkv=3)), ("Sk = 0", dict(Sk=0)),
                     ("Sk = 192", dict(Sk=192)), ("Sk = 16512", dict(Sk=16512)), ("head_dim 32", dict(D=32)), ("head_dim 96", dict(D=96)),
                     ("both outputs NULL", dict(none=True)), ("a misaligned out", dict(out_off=8)), ("a misaligned out8", dict(out8_off=8)),
                     ("B * Hkv = 65536", dict(B=ac.REFUSED_BH, H=2, Hkv=1))):
        refused(lambda g: call(g, **kw), spec, what)


@pytest.mark.parametrize("switch", ["1", None])
def test_attention_fp8_gqa_route(nv, monkeypatch, switch):
    """One quantized layer of llama-gqa-tiny (4 query heads of 64 over 2 kv heads, stateless E4M3, 2 x 128 tokens, no KV cache): under
    QT_FUSED_ATTENTION=1, or where _fp8_gqa_route_takes lists the shape, the layer calls qt_attention_fp8_gqa once with Hkv = 2,
    _repeat_kv makes no copy, the block returns that launch's bits and routes_report names the route; otherwise the entry point is not
    called and the path repeats as before."""
    import quantized_training as qt
    from quantized_training import attention_route, fused, handover
    from quantized_training.harness import build_causal_lm
    from quantized_training.modules.quantizable import attention as quantizable_attention
    B, H, Hkv, S, D = 2, 4, 2, 128, 64
    monkeypatch.delenv("QT_FUSED_ATTENTION", raising=False)
    if switch:
        monkeypatch.setenv("QT_FUSED_ATTENTION", switch)
    taken = bool(switch) or attention_route._fp8_gqa_route_takes(B, H, Hkv, S, S, D)
    attention_route.ATTENTION_ROUTES.clear()
    quantizable_attention._CAUSAL.clear()
    L, calls, returned, repeats = nv.lib(), [], [], []
    fn = L.qt_attention_fp8_gqa

    def spy(*args):                                                         # the entry point again on the same codes, into buffers of its own
        out = torch.empty((B, S, H, D), dtype=torch.bfloat16, device="cuda") if args[14] else None
        out8 = torch.empty((B, S, H, D), dtype=torch.uint8, device="cuda") if args[15] else None
        assert fn(*args[:14], _ptr(out), _ptr(out8), *args[16:]) == 0
        calls.append((args[19], out, out8))
        return fn(*args)

    real, real_repeat = attention_route._attention_fp8_or_none, quantizable_attention._repeat_kv
    monkeypatch.setattr(attention_route, "_attention_fp8_or_none", lambda *a: returned.append(real(*a)) or returned[-1])
    monkeypatch.setattr(quantizable_attention, "_repeat_kv", lambda t, n: repeats.append(n) or real_repeat(t, n))
    m = build_causal_lm("llama-gqa-tiny", num_layers=1).eval()
    qt.quantize(m, qt.add_qspec_args().parse_args(["--activation", "e4m3", "--weight", "e4m3", "--bf16"]))
    ids = torch.randint(3, 512, (B, S), generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        m(ids, use_cache=False)                                             # the first call creates the fake-quantizers
        del returned[:], repeats[:]
        monkeypatch.setattr(L, "qt_attention_fp8_gqa", spy)
        m(ids, use_cache=False)
        torch.cuda.synchronize()
    assert [c[0] for c in calls] == ([Hkv] if taken else []), calls
    assert repeats == ([] if taken else [2, 2])
    assert (fused.routes_report().get(f"attention:{B}x{H}x{Hkv}x{S}x{S}x{D}") == "attention_fp8_gqa") == taken
    if taken:
        (_, out, out8), got = calls[0], returned[-1]
        assert got is not None and (out is not None or out8 is not None)
        assert out is None or torch.equal(got.view(torch.int16), out.view(torch.int16))
        assert out8 is None or torch.equal(handover.codes(got, unchecked=True).view(torch.uint8), out8)
