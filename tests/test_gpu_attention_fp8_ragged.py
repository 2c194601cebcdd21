"""qt_value_codes_t_ragged + qt_attention_fp8_ragged (csrc/qt_attention_fp8_ragged.hip; head_dim 64 / 128, any key count 1 .. 512): through the C
ABI into guarded buffers against the interval oracle's "strip_fp8" model (v holds one key per column: every output is one exact product), and
through one BERT layer at 197 tokens."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import attention_cases as ac
from oracle import qt_oracle as o

from kernel_launch import Guarded, dev, inside, launch, nv, refused, same, stream  # noqa: F401
from test_gpu_attention_cores import Inputs, _bhsd, _fp8_codes, _fp8_tables, _ptr

pytestmark = pytest.mark.gpu

# name: (B, H, Sq, Sk, D, format, mask(rng) or None, live, mask row stride or None)
CASES = {
    "sq197_sk197_d64_e4m3_nomask": (1, 2, 197, 197, 64, "e4m3", None, False, None),
    "sq1_sk1_d64_e4m3_nomask": (1, 2, 1, 1, 64, "e4m3", None, False, None),
    "sq65_sk68_d64_e5m2_bias": (1, 2, 65, 68, 64, "e5m2", lambda r: ac.bias((1, 2, 65, 68), r), False, 71),     # rows Sk + 3 apart, +inf between
    "sq65_sk129_d128_e5m2_padding": (2, 2, 65, 129, 128, "e5m2", lambda r: ac.padding([129, 77], 129), True, None),
    "sq65_sk200_d128_e4m3_ragged": (1, 2, 65, 200, 128, "e4m3", lambda r: ac.ragged(65, 200, r), True, None),
    "sq130_sk385_d128_e4m3_causal": (1, 1, 130, 385, 128, "e4m3", lambda r: ac.causal(130, 385), True, None),
    "sq65_sk511_d64_e4m3_hole": (1, 2, 65, 511, 64, "e4m3", lambda r: ac.hole(65, 511, 40, 300), True, None),
    "sq65_sk197_d64_e4m3_padding0": (2, 1, 65, 197, 64, "e4m3", lambda r: ac.padding([197, 0], 197), True, None),
}
KEY_OF = (np.arange(128) & 64) | (((np.arange(128) >> 2) & 3) << 4) | (((np.arange(128) >> 4) & 3) << 2) | (np.arange(128) & 3)   # slot p holds key KEY_OF[p]


def _ragged(nv, c, x, q8, k8, vt8, fmt, out, out8, live=False, simple=0, flag=False):
    """One launch: mask read, or (live) the row extents with the caller's verdict (simple) or the device's (flag)."""
    rl, ls = (x.rl, x.ls) if live else (None, (0, 0, 0))
    return nv.lib().qt_attention_fp8_ragged(q8.data_ptr(), k8.data_ptr(), vt8.data_ptr(), 0 if c.fmt == "e4m3" else 1, _ptr(x.mask), *x.ms, rl, *ls, simple,
                                            x.irr if flag else None, out, out8, ctypes.byref(fmt) if out8 else None, c.B, c.H, c.Sq, c.Sk, c.D, c.scaling, stream())


@pytest.mark.parametrize("name", list(CASES))
def test_attention_fp8_ragged_every_variant(nv, name):
    """Inside the interval; the output modes and the mask forms bit-equal; guards intact (launch); V^T's pad slots 0; one graph replay bit-equal."""
    B, H, Sq, Sk, D, fmt_name, mask, live, row_stride = CASES[name]
    q, k, v, rng = ac._qkv(name, B, H, Sq, Sk, D)
    c = ac.Case(name, "fp8", q, k, ac.one_key_per_column(v), None if mask is None else mask(rng), row_stride=row_stride, fmt=fmt_name, live=live)
    iv, ivq = c.intervals(), c.intervals(out_fq=True)
    share, nonzero = iv.out.decided_share(), float(((iv.out.lo & 0x7FFF) != 0).mean())
    print(f"\n[{name}] decided {share:.4f}, non-zero {nonzero:.3f}")
    assert share >= 0.99 and nonzero >= 0.15, "the case decides too little"
    x = Inputs(nv, c)
    fmt = nv.format_for(c.fmt)
    q8, k8 = dev(_fp8_codes(c.q, c.fmt)), dev(_fp8_codes(c.k, c.fmt))
    nkb = (Sk + 127) // 128
    vt = launch(lambda g: nv.lib().qt_value_codes_t_ragged(x.v.data_ptr(), g["vt8"].ptr, B, H, Sk, D, H * Sk * D, Sk * D, D, ctypes.byref(fmt), stream()),
                {"vt8": ((B, H, D, 128 * nkb), np.uint8)}, f"qt_value_codes_t_ragged {name}")["vt8"]      # (its layout is checked through the core)
    pad = (128 * np.arange(nkb)[:, None] + KEY_OF[None, :]).reshape(-1) >= Sk
    assert pad.sum() == 128 * nkb - Sk and not vt[..., pad].any(), "the slots of the keys >= Sk hold code 0"
    vt8 = dev(vt)
    shape = (c.B, c.Sq, c.H, c.D)

    def run(mode, what, **kw):
        specs = {k: (shape, t) for k, t in (("out", np.uint16), ("out8", np.uint8)) if mode in (k, "both")}
        return launch(lambda g: _ragged(nv, c, x, q8, k8, vt8, fmt, g["out"].ptr if "out" in g else None, g["out8"].ptr if "out8" in g else None, **kw), specs, what)

    what = f"qt_attention_fp8_ragged {name}"
    r0 = run("out", what)
    inside(iv.out, _bhsd(r0["out"]), what, "attention_fp8_ragged")
    rb = run("both", what + " out + out8")
    inside(ivq.out, _bhsd(rb["out"]), what + " out + out8", "attention_fp8_ragged")
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
    g_out, side, graph = Guarded(shape, np.uint16), torch.cuda.Stream(), torch.cuda.CUDAGraph()       # one graph replay against the eager result
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        assert _ragged(nv, c, x, q8, k8, vt8, fmt, g_out.ptr, None, live=c.live, flag=c.live) == 0
    graph.replay()
    torch.cuda.synchronize()
    assert g_out.intact()
    same(g_out.host(), r0["out"], what + ": graph replay / eager")


def test_attention_fp8_ragged_refusals(nv):
    """What the entry point does not take: an error status, nothing written.  qt_attention_fp8 keeps refusing 197 keys."""
    fmt, big = nv.format_for("e4m3"), dev(np.zeros(2 * 640 * 128, np.uint8))
    spec = {"out": ((1, 65, 2, 128), np.uint16), "out8": ((1, 65, 2, 128), np.uint8)}

    def call(g, entry="qt_attention_fp8_ragged", B=1, H=2, Sk=197, D=64, out_off=0, out8_off=0, none=False):
        out, out8 = (None, None) if none else (g["out"].ptr + out_off, g["out8"].ptr + out8_off)
        return getattr(nv.lib(), entry)(big.data_ptr(), big.data_ptr(), big.data_ptr(), 0, None, 0, 0, 0, None, 0, 0, 0, 0, None, out, out8,
                                        ctypes.byref(fmt), B, H, 65, Sk, D, D ** -0.5, stream())

    for what, kw in (("Sk = 0", dict(Sk=0)), ("Sk = 513", dict(Sk=513)), ("head_dim 32", dict(D=32)), ("head_dim 96", dict(D=96)),
                     ("both outputs NULL", dict(none=True)), ("a misaligned out", dict(out_off=8)), ("a misaligned out8", dict(out8_off=8)),
                     ("B * H = 65536", dict(B=ac.REFUSED_BH, H=1)), ("qt_attention_fp8 at Sk = 197", dict(entry="qt_attention_fp8"))):
        refused(lambda g: call(g, **kw), spec, what)


@pytest.mark.parametrize("switch", ["1", None])
def test_attention_fp8_ragged_route(nv, monkeypatch, switch):
    """One quantized BERT layer (2 heads of 64, stateless E4M3, 4 x 197 tokens, one sample padded from 150 on): the layer calls
    qt_attention_fp8_ragged once (routes_report names it) and the block returns its bits -- under QT_FUSED_ATTENTION=1, and without it
    as _fp8_ragged_route_takes says."""
    import quantized_training as qt
    from quantized_training import attention_route, fused
    from transformers import BertConfig, BertModel
    B, H, S = 4, 2, 197
    monkeypatch.delenv("QT_FUSED_ATTENTION", raising=False)
    if switch:
        monkeypatch.setenv("QT_FUSED_ATTENTION", switch)
    core = "qt_attention_fp8_ragged" if switch or attention_route._fp8_ragged_route_takes(B, H, S, S, 64) else None
    attention_route.ATTENTION_ROUTES.clear()
    L, calls, returned = nv.lib(), [], []

    def spy(name, fn):
        def wrapped(*args):                                                 # the entry point again on the same codes, into buffers of its own
            out = torch.empty((B, S, H, 64), dtype=torch.bfloat16, device="cuda") if args[14] else None
            out8 = torch.empty((B, S, H, 64), dtype=torch.uint8, device="cuda") if args[15] else None
            assert fn(*args[:14], _ptr(out), _ptr(out8), *args[16:]) == 0
            calls.append((name, out))
            return fn(*args)
        monkeypatch.setattr(L, name, wrapped)

    real = attention_route._attention_fp8_or_none
    monkeypatch.setattr(attention_route, "_attention_fp8_or_none", lambda *a: returned.append(real(*a)) or returned[-1])
    torch.manual_seed(0)
    m = BertModel(BertConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=H, intermediate_size=256, vocab_size=300,
                             max_position_embeddings=S)).eval().bfloat16().cuda()
    qt.quantize(m, qt.add_qspec_args().parse_args(["--activation", "e4m3", "--weight", "e4m3", "--bf16"]))
    ids = torch.randint(3, 300, (B, S), generator=torch.Generator().manual_seed(2)).cuda()
    att = torch.ones_like(ids)
    att[1, 150:] = 0
    with torch.no_grad():
        m(ids, attention_mask=att)                                          # the first call creates the fake-quantizers
        for name in ("qt_attention_fp8", "qt_attention_fp8_long", "qt_attention_fp8_ragged"):
            spy(name, getattr(L, name))
        m(ids, attention_mask=att)
    assert [c[0] for c in calls] == ([core] if core else []), calls
    assert (fused.routes_report().get(f"attention:{B}x{H}x{S}x{S}x64") == "attention_fp8_ragged") == (core is not None)
    if core:
        assert torch.equal(returned[-1].view(torch.int16), calls[0][1].view(torch.int16))       # (BertSelfOutput's block: never codes only)
