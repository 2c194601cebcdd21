"""qt_attention_fp8's three output modes through the C ABI -- values only, values + codes, codes only -- and the codes-only hand-over
of the attention core to the output projection at model level.

The kernel's epilogue lets both wave groups finish half of the 64 x D tile, turns the tile round in LDS and stores 16 bytes a lane;
the shapes are the smallest at which each of its paths can go wrong (one key-block pair with a dead second block, a ragged last block of
query rows, the full four-pair strip, head_dim 64 with the 512-key instantiation and the mask-read path, both operand and both consumer
formats).  Per case the oracle's result is computed once and all three modes are held against it."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import qt_oracle as o

pytestmark = pytest.mark.gpu

F8_TORCH = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
SENTINEL16, SENTINEL8 = 0x7FA5, 0xA5            # a NaN pattern no rounding produces / a code the poison of nothing else uses


@pytest.fixture(scope="module")
def nv():
    from quantized_training import _native
    assert torch.cuda.is_available(), "these tests need the GPU"
    _native.lib()
    return _native


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def host_u16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _codes_of(nv, t, dtype):
    """FP8 codes of fq(t) from the (oracle-pinned) elementwise pass, as a uint8 device tensor."""
    fmt = nv.format_for(dtype)
    y8 = torch.empty(t.shape, dtype=torch.uint8, device="cuda")
    one = torch.ones((), dtype=torch.float32, device="cuda")
    nv.check(nv.lib().qt_fake_quant_bf16_fp8(t.data_ptr(), None, y8.data_ptr(), t.numel(), ctypes.byref(fmt), one.data_ptr(), None, stream()), "fq8")
    return y8


def _oracle_codes(bits, dtype):
    """The oracle's closed-form fake-quantization of bf16 values (uint16 bits), turned into FP8 codes: its results lie on the format's
    grid, where the conversion to torch's FP8 type is exact (sign of zero included)."""
    f = o.quantize_to_fp8_e4m3 if dtype == "e4m3" else o.quantize_to_fp8_e5m2
    return torch.from_numpy(f(o.bf16_to_f32(bits))).to(F8_TORCH[dtype]).view(torch.uint8).numpy()


class _Guarded:
    """A [B, Sq, H, D] tensor inside a larger sentinel-filled buffer: 64 rows of H x D elements in front of it and behind it (the rows a
    ragged last block of query rows would reach if the kernel stored them)."""

    def __init__(self, shape, dtype):
        B, Sq, H, D = shape
        self.pad, self.n = 64 * H * D, B * Sq * H * D
        self.sentinel = SENTINEL16 if dtype == torch.bfloat16 else SENTINEL8
        raw = torch.int16 if dtype == torch.bfloat16 else torch.uint8
        self.buf = torch.full((self.n + 2 * self.pad,), self.sentinel, dtype=torch.int32, device="cuda").to(raw)
        self.t = self.buf[self.pad:self.pad + self.n].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0

    def sentinels_intact(self):
        return bool((self.buf[:self.pad] == self.sentinel).all()) and bool((self.buf[self.pad + self.n:] == self.sentinel).all())


# (D, B, H, Sq, Sk, mask kind, operand format, consumer format)
CASES = [
    (128, 1, 2, 256, 256, "causal", "e4m3", "e4m3"),       # one key-block pair; its second block is dead for the first query blocks
    (128, 1, 1, 200, 256, None, "e4m3", "e4m3"),           # ragged last block of query rows: 8 rows
    (128, 1, 1, 1024, 1024, "causal", "e4m3", "e4m3"),     # the full four-pair strip
    (64, 2, 3, 384, 384, None, "e4m3", "e4m3"),            # head_dim 64, the 512-key instantiation (two workgroups per CU)
    (64, 2, 3, 384, 384, "padding", "e4m3", "e4m3"),       # ... with a right-padding additive mask that the kernel reads
    (128, 1, 2, 256, 256, "causal", "e5m2", "e4m3"),       # E5M2 operands
    (128, 1, 2, 256, 256, "causal", "e4m3", "e5m2"),       # an E5M2 consumer
]


@pytest.mark.parametrize("D,B,H,Sq,Sk,mask_kind,fmt_name,out_fmt_name", CASES)
def test_attention_fp8_output_modes(nv, D, B, H, Sq, Sk, mask_kind, fmt_name, out_fmt_name):
    """Values only, values + codes and codes only from the same inputs.  The plain values meet the bounds of
    test_gpu_parity.py::test_attention_fp8_kernel against oracle.attention_fq (restated, not loosened); with a consumer format the values
    are the oracle's fake-quantization of the plain values and the codes its codes, bit for bit; codes only writes the same codes and
    nothing else; no mode touches a byte outside rows 0 .. Sq-1 of its buffers.  (With a consumer format `out` holds fq(result), so the
    first two modes' values are equal exactly where the consumer's rounding is the identity; the assertion is the stronger one: every
    value of the second mode is the oracle's fake-quantization of the first mode's.)"""
    L = nv.lib()
    torch.manual_seed(D + 3 * Sq + Sk + H)
    qmap_in = torch.from_numpy(o.get_quantization_map(fmt_name).view(np.int16)).cuda().view(torch.bfloat16)
    fqin = lambda t: qmap_in[(t.view(torch.int16).to(torch.int32) & 0xFFFF).long()]  # noqa: E731
    q = fqin(torch.randn(B, H, Sq, D, device="cuda").bfloat16())
    k = fqin(torch.randn(B, H, Sk, D, device="cuda").bfloat16())
    v_raw = torch.randn(B, Sk, H, D, device="cuda").bfloat16().transpose(1, 2)
    v = fqin(v_raw.contiguous())
    scaling = D ** -0.5
    minv = torch.finfo(torch.bfloat16).min
    mask, msb, msq, rl_ptr, lsq, flag = None, 0, 0, None, 0, None
    if mask_kind == "causal":
        # as the model issues it: row extents and the device's verdict on the mask's rows; the mask itself is then not read
        mask = torch.full((Sq, Sk), minv, device="cuda").triu(1 + Sk - Sq).bfloat16()[None, None]
        msq = mask.stride(2)
        rl = torch.empty(Sq + 1, dtype=torch.int32, device="cuda")
        nv.check(L.qt_mask_row_live_checked(mask.data_ptr(), Sq, Sk, Sk, rl.data_ptr(), rl.data_ptr() + 4 * Sq, stream()), "qt_mask_row_live_checked")
        assert int(rl[-1]) == 0
        rl_ptr, lsq, flag = rl.data_ptr(), 1, rl.data_ptr() + 4 * Sq
    elif mask_kind == "padding":
        # no extents: the kernel reads the mask
        mask = torch.zeros(B, 1, 1, Sk, device="cuda", dtype=torch.bfloat16)
        mask[:, :, :, Sk - 29:] = minv
        mask[0, :, :, Sk - 150:] = minv
        msb = mask.stride(0)
    fmt, fo = nv.format_for(fmt_name), nv.format_for(out_fmt_name)
    fcode = 0 if fmt_name == "e4m3" else 1
    q8, k8 = _codes_of(nv, q, fmt_name), _codes_of(nv, k, fmt_name)
    vt8 = torch.empty(B, H, D, Sk, dtype=torch.uint8, device="cuda")
    nv.check(L.qt_value_codes_t(v_raw.data_ptr(), vt8.data_ptr(), B, H, Sk, D, v_raw.stride(0), v_raw.stride(1), v_raw.stride(2), ctypes.byref(fmt),
                                stream()), "qt_value_codes_t")

    def launch(out, out8):
        return L.qt_attention_fp8(q8.data_ptr(), k8.data_ptr(), vt8.data_ptr(), fcode, mask.data_ptr() if mask is not None else None, msb, 0, msq,
                                  rl_ptr, 0, 0, lsq, 0, flag, out.t.data_ptr() if out is not None else None,
                                  out8.t.data_ptr() if out8 is not None else None, ctypes.byref(fo) if out8 is not None else None,
                                  B, H, Sq, Sk, D, scaling, stream())

    shape = (B, Sq, H, D)
    plain = _Guarded(shape, torch.bfloat16)                                                   # mode 1: values only
    both_v, both_c = _Guarded(shape, torch.bfloat16), _Guarded(shape, torch.uint8)          # mode 2: values + codes
    only_c = _Guarded(shape, torch.uint8)                                                     # mode 3: codes only
    nv.check(launch(plain, None), "qt_attention_fp8")
    nv.check(launch(both_v, both_c), "qt_attention_fp8")
    nv.check(launch(None, only_c), "qt_attention_fp8")
    assert launch(None, None) == nv.QT_ERR_BAD_ARG
    torch.cuda.synchronize()
    for g in (plain, both_v, both_c, only_c):
        assert g.sentinels_intact()        # in front of row 0 and behind row Sq - 1: the rows of a ragged last block that do not exist

    # the plain values against the oracle: the bounds of test_gpu_parity.py::test_attention_fp8_kernel
    u16 = lambda t: host_u16(t)  # noqa: E731
    exp, _ = o.attention_fq(u16(q), u16(k), u16(v), u16(mask) if mask is not None else None, scaling, o.get_quantization_map(fmt_name))
    got = u16(plain.t.permute(0, 2, 1, 3))
    share = float((got != exp).mean())
    ev = o.bf16_to_f32(exp)
    err = float((np.abs(o.bf16_to_f32(got) - ev) / (np.abs(ev).max(axis=-1, keepdims=True) + 1e-30)).max())
    l2 = float(np.sqrt(((o.bf16_to_f32(got).astype(np.float64) - ev) ** 2).sum() / ((ev.astype(np.float64) ** 2).sum() + 1e-30)))
    print(f"share of differing elements {share:.3e}, largest row-relative error {err:.3e}, relative l2 {l2:.3e}")
    assert share <= (1.2e-2 if fmt_name == "e4m3" else 3e-2), share
    assert err <= 0.08, err
    assert l2 <= (4e-3 if fmt_name == "e4m3" else 1.2e-2), l2

    # with the consumer's format: the oracle's fake-quantization of the kernel's own plain values, and its codes
    plain_bits = host_u16(plain.t)
    want_v = o.vmap_bf16(plain_bits, o.get_quantization_map(out_fmt_name))
    want_c = _oracle_codes(plain_bits, out_fmt_name)
    assert np.array_equal(host_u16(both_v.t), want_v)
    assert np.array_equal(both_c.t.cpu().numpy(), want_c)
    assert np.array_equal(only_c.t.cpu().numpy(), want_c)


def test_attention_fp8_refuses_unaligned_outputs(nv):
    """Both results leave in 16-byte stores: a pointer that is not 16-byte aligned is QT_ERR_UNALIGNED, before anything is launched."""
    L = nv.lib()
    B, H, S, D = 1, 1, 128, 128
    z8 = torch.zeros(B * H * S * D + 64, dtype=torch.uint8, device="cuda")
    o8 = torch.zeros(B * H * S * D + 64, dtype=torch.uint8, device="cuda")
    z16 = torch.zeros(B * H * S * D + 64, dtype=torch.int16, device="cuda")
    fo = nv.format_for("e4m3")

    def launch(out_ptr, out8_ptr):
        return L.qt_attention_fp8(z8.data_ptr(), z8.data_ptr(), z8.data_ptr(), 0, None, 0, 0, 0, None, 0, 0, 0, 0, None, out_ptr, out8_ptr,
                                  ctypes.byref(fo), B, H, S, S, D, 0.1, stream())
    assert launch(z16.data_ptr() + 8, o8.data_ptr()) == nv.QT_ERR_UNALIGNED
    assert launch(z16.data_ptr(), o8.data_ptr() + 4) == nv.QT_ERR_UNALIGNED
    assert launch(None, o8.data_ptr() + 8) == nv.QT_ERR_UNALIGNED
    assert launch(z16.data_ptr(), o8.data_ptr()) == 0
    torch.cuda.synchronize()


# ---- model level: the codes-only hand-over to the output projection changes nothing -------------------------------------------------------
def _tiny_llama():
    pytest.importorskip("transformers")
    import quantized_training as qt
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, vocab_size=512,
                      max_position_embeddings=256, attn_implementation="eager")
    m = LlamaForCausalLM(cfg).eval().to(device="cuda", dtype=torch.bfloat16)
    qt.quantize(m, qt.add_qspec_args().parse_args(["--activation", "e4m3", "--weight", "e4m3", "--bf16", "--quantize_forward", "gemm"]))
    return m


def test_codes_only_attention_leaves_the_window_nll_unchanged(monkeypatch):
    """A 2-layer LLaMA (hidden 256, 2 heads of 128): the window NLL with the attention core handing only codes to o_proj
    (QT_CODES_ONLY=1) and with every producer writing values (=0) is the same number bit for bit, eager and through GraphedWindow.  The
    suite runs with QT_LAZY_POISON=1: a read of the unwritten values would surface as NaN."""
    from quantized_training import attention_route, harness
    ids = torch.randint(0, 512, (1, 256), generator=torch.Generator().manual_seed(5)).cuda()
    res, lazy_seen = {}, {}
    real = attention_route.attention_output_plan

    for mode in ("1", "0"):
        monkeypatch.setenv("QT_CODES_ONLY", mode)
        seen = []
        monkeypatch.setattr(attention_route, "attention_output_plan", lambda attn, seen=seen: (seen.append(real(attn)), seen[-1])[1])
        m = _tiny_llama()
        with torch.no_grad():
            harness.window_nll(m, ids, 256)                                  # the first call creates the fake-quantizers
            eager = harness.window_nll(m, ids, 256)
            g = harness.GraphedWindow(m, 256, None, torch.device("cuda"))
            g.capture(ids)
            graphed = g.replay(ids, 256)
        res[mode] = (torch.as_tensor(eager).float().cpu(), torch.as_tensor(graphed).float().cpu())
        lazy_seen[mode] = [codes_only for _, codes_only in seen]
    assert lazy_seen["1"] and any(lazy_seen["1"]), "the FP8 attention core ran and handed codes only"
    assert lazy_seen["0"] and not any(lazy_seen["0"])
    for a, b in zip(res["1"], res["0"]):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (a, b)
