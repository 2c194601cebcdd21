"""qt_attention_fp8_long (csrc/qt_attention_fp8_long.hip), the streaming two-sweep FP8 attention core for 128 .. 16384 keys: through the
C ABI into guarded buffers against the interval oracle's "online" model (a running maximum that advances per key block), and through the
module route.  v holds one key per column (oracle/attention_cases.py): every output is one exact product, compared to the bit."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import attention_cases as ac
from oracle import qt_oracle as o

from kernel_launch import Guarded, dev, inside, launch, nv, refused, same, stream  # noqa: F401
from test_gpu_attention_cores import Inputs, _bhsd, _fp8_codes, _fp8_tables, _fp8_value_pass, _ptr

pytestmark = pytest.mark.gpu


def _steps(Sq, Sk, rising):
    """One unit of bias per 128-key block: every row's maximum in the last block (rising at every block) or in the first."""
    kb = np.arange(Sk) // 128
    row = (kb - kb.max() if rising else -kb).astype(np.float64)
    return np.broadcast_to(ac._bits(row), (1, 1, Sq, Sk)).copy()


# name: (B, H, Sq, Sk, D, format, mask(rng) or None, live)
CASES = {
    "sq65_sk1152_d128_e4m3_nomask": (1, 2, 65, 1152, 128, "e4m3", None, False),
    "sq130_sk1536_d64_e5m2_ragged": (1, 2, 130, 1536, 64, "e5m2", lambda r: ac.ragged(130, 1536, r), True),
    "sq1_sk2048_d128_e5m2_bias": (1, 2, 1, 2048, 128, "e5m2", lambda r: ac.bias((1, 2, 1, 2048), r), False),
    "sq65_sk1280_d64_e5m2_padding": (2, 1, 65, 1280, 64, "e5m2", lambda r: ac.padding([1280, 1100], 1280), True),
    "sq65_sk2048_d128_e5m2_hole": (1, 2, 65, 2048, 128, "e5m2", lambda r: ac.hole(65, 2048, 200, 1900), True),
    "sq1152_sk1152_d128_e4m3_causal": (1, 1, 1152, 1152, 128, "e4m3", lambda r: ac.causal(1152, 1152), True),
    "sq65_sk1280_d128_e5m2_max_last": (1, 2, 65, 1280, 128, "e5m2", lambda r: _steps(65, 1280, True), False),
    "sq65_sk1280_d64_e5m2_max_first": (1, 2, 65, 1280, 64, "e5m2", lambda r: _steps(65, 1280, False), False),
    "sq65_sk256_d64_e4m3_ragged": (1, 2, 65, 256, 64, "e4m3", lambda r: ac.ragged(65, 256, r), True),
}


def make_case(name):
    B, H, Sq, Sk, D, fmt, mask, live = CASES[name]
    q, k, v, rng = ac._qkv(name, B, H, Sq, Sk, D)
    c = ac.Case(name, "fp8", q, k, ac.one_key_per_column(v), None if mask is None else mask(rng), fmt=fmt, live=live)
    c.kernel = "online"
    return c


def _long(nv, c, x, q8, k8, vt8, fmt, out, out8, live=False, simple=0, flag=False):
    """One launch: mask read, or (live) the row extents with the caller's verdict (simple) or the device's (flag)."""
    rl, ls = (x.rl, x.ls) if live else (None, (0, 0, 0))
    return nv.lib().qt_attention_fp8_long(q8.data_ptr(), k8.data_ptr(), vt8.data_ptr(), 0 if c.fmt == "e4m3" else 1, _ptr(x.mask), *x.ms, rl, *ls, simple,
                                          x.irr if flag else None, out, out8, ctypes.byref(fmt) if out8 else None, c.B, c.H, c.Sq, c.Sk, c.D, c.scaling, stream())


@pytest.mark.parametrize("name", list(CASES))
def test_attention_fp8_long_every_variant(nv, name):
    """Inside the interval; the output modes and the mask forms bit-equal; guards intact (launch); one graph replay bit-equal."""
    c = make_case(name)
    iv, ivq = c.intervals(), c.intervals(out_fq=True)
    share, nonzero = iv.out.decided_share(), float(((iv.out.lo & 0x7FFF) != 0).mean())
    print(f"\n[{name}] decided {share:.4f}, non-zero {nonzero:.3f}")
    assert share >= 0.99 and nonzero >= 0.15, "the case decides too little"
    x = Inputs(nv, c)
    fmt = nv.format_for(c.fmt)
    q8, k8 = dev(_fp8_codes(c.q, c.fmt)), dev(_fp8_codes(c.k, c.fmt))
    vt8 = _fp8_value_pass(nv, c, x, fmt)
    shape = (c.B, c.Sq, c.H, c.D)
    decode = _fp8_tables(c.fmt)

    def run(mode, what, **kw):
        specs = {k: (shape, t) for k, t in (("out", np.uint16), ("out8", np.uint8)) if mode in (k, "both")}
        return launch(lambda g: _long(nv, c, x, q8, k8, vt8, fmt, g["out"].ptr if "out" in g else None, g["out8"].ptr if "out8" in g else None, **kw), specs, what)

    what = f"qt_attention_fp8_long {name}"
    r0 = run("out", what)
    inside(iv.out, _bhsd(r0["out"]), what, "attention_fp8_long")
    rb = run("both", what + " out + out8")
    inside(ivq.out, _bhsd(rb["out"]), what + " out + out8", "attention_fp8_long")
    same(rb["out"], o.vmap_bf16(r0["out"], c.qmap()), what + ": out is the map of the plain result")
    same(decode[rb["out8"]], rb["out"], what + ": the codes decode to out")
    same(run("out8", what + " codes only")["out8"], rb["out8"], what + ": codes only / out + out8")
    if c.live:
        forms = [("row extents", dict(simple=0)), ("device flag", dict(flag=True))]
        if not x.irregular:
            forms.append(("mask_is_simple", dict(simple=1)))
        for tag, kw in forms:
            same(run("out", f"{what} {tag}", live=True, **kw)["out"], r0["out"], f"{what}: {tag} / mask read")
        same(run("out8", what + " device flag, codes only", live=True, flag=True)["out8"], rb["out8"], what + ": device flag, codes only")
    # one captured-graph replay against the eager result
    g_out = Guarded(shape, np.uint16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        assert _long(nv, c, x, q8, k8, vt8, fmt, g_out.ptr, None, live=c.live, flag=c.live) == 0
    graph.replay()
    torch.cuda.synchronize()
    assert g_out.intact()
    same(g_out.host(), r0["out"], what + ": graph replay / eager")


def test_attention_fp8_long_refusals(nv):
    """What the entry point does not take: an error status, nothing written."""
    c = make_case("sq65_sk256_d64_e4m3_ragged")
    fmt = nv.format_for(c.fmt)
    big = dev(np.zeros(c.B * c.H * 1280 * 128, np.uint8))
    spec = {"out": ((c.B, c.Sq, c.H, c.D), np.uint16), "out8": ((c.B, c.Sq, c.H, c.D), np.uint8)}

    def call(g, B=c.B, H=c.H, Sk=c.Sk, D=c.D, out_off=0, out8_off=0, none=False):
        out, out8 = (None, None) if none else (g["out"].ptr + out_off, g["out8"].ptr + out8_off)
        return nv.lib().qt_attention_fp8_long(big.data_ptr(), big.data_ptr(), big.data_ptr(), 0, None, 0, 0, 0, None, 0, 0, 0, 0, None, out, out8,
                                              ctypes.byref(fmt), B, H, c.Sq, Sk, D, c.scaling, stream())

    for Sk in (64, 1152 + 64, 16512):
        refused(lambda g: call(g, Sk=Sk), spec, f"Sk = {Sk}")
    for what, kw in (("head_dim 32", dict(D=32)), ("both outputs NULL", dict(none=True)), ("a misaligned out", dict(out_off=8)),
                     ("a misaligned out8", dict(out8_off=8)), ("B * H = 65536", dict(B=ac.REFUSED_BH, H=1))):
        refused(lambda g: call(g, **kw), spec, what)


@pytest.mark.parametrize("S,switch,core", [(1152, "1", "qt_attention_fp8_long"), (1152, None, None), (1024, "1", "qt_attention_fp8")])
def test_attention_fp8_long_route(nv, monkeypatch, S, switch, core):
    """One quantized LLaMA layer (2 heads of 64, stateless E4M3, causal): under QT_FUSED_ATTENTION=1 1152 keys take the new core
    (routes_report names it) and the block returns what the entry point gives on the same codes; without the switch the route is what
    _fp8_long_route_takes says; 1024 keys stay with qt_attention_fp8."""
    import quantized_training as qt
    from quantized_training import attention_route, fused, handover
    from quantized_training.modules.quantizable import attention as quantizable_attention
    from transformers import LlamaConfig, LlamaModel
    if switch is None:
        monkeypatch.delenv("QT_FUSED_ATTENTION", raising=False)
        core = "qt_attention_fp8_long" if attention_route._fp8_long_route_takes(1, 2, S, S, 64) else None
    else:
        monkeypatch.setenv("QT_FUSED_ATTENTION", switch)
    attention_route.ATTENTION_ROUTES.clear()
    quantizable_attention._CAUSAL.clear()
    L = nv.lib()
    calls, returned = [], []

    def spy(name, fn):
        def wrapped(*args):                                                 # the entry point again on the same codes, into buffers of its own
            out = torch.empty((1, S, 2, 64), dtype=torch.bfloat16, device="cuda") if args[14] else None
            out8 = torch.empty((1, S, 2, 64), dtype=torch.uint8, device="cuda") if args[15] else None
            assert fn(*args[:14], _ptr(out), _ptr(out8), *args[16:]) == 0
            calls.append((name, out, out8))
            return fn(*args)
        monkeypatch.setattr(L, name, wrapped)

    real = attention_route._attention_fp8_or_none
    monkeypatch.setattr(attention_route, "_attention_fp8_or_none", lambda *a: returned.append(real(*a)) or returned[-1])
    torch.manual_seed(0)
    m = LlamaModel(LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
                               vocab_size=320, max_position_embeddings=S)).eval().bfloat16().cuda()
    qt.quantize(m, qt.add_qspec_args().parse_args(["--activation", "e4m3", "--weight", "e4m3", "--bf16"]))
    ids = torch.randint(3, 320, (1, S), generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        m(ids, use_cache=False)                                             # the first call creates the fake-quantizers
        del returned[:]
        for name in ("qt_attention_fp8", "qt_attention_fp8_long"):
            spy(name, getattr(L, name))
        m(ids, use_cache=False)
        torch.cuda.synchronize()
    assert [c[0] for c in calls] == ([core] if core else []), calls
    assert (fused.routes_report().get(f"attention:1x2x{S}x{S}x64") == "attention_fp8_long") == (core == "qt_attention_fp8_long")
    if core:
        (_, out, out8), got = calls[0], returned[-1]
        assert got is not None and (out is not None or out8 is not None)
        assert out is None or torch.equal(got.view(torch.int16), out.view(torch.int16))
        assert out8 is None or torch.equal(handover.codes(got, unchecked=True).view(torch.uint8), out8)
