"""The block-scaled float attention core (qt_attention_mxf) behind attention_mx against the chain of the six nodes it replaces
(csrc/qt_attention_mxf.hip's header) on the CPU: operands dequantized to float64, sums and the softmax in float64, the stated roundings,
P through the CPU quantize_mx.  Exact tier, bit for bit: one-hot rows, uniform rows over integer V, and the read-out (V an identity
window: the output is P' there) wherever the reference's p is firm.  The read-out's q and k are small integers: the instruction's fp32
sum over head_dim is then exact and the bf16 logits are the reference's own (profiles/attention_mxf.txt has the count without that).
The kernel's p differs from the reference's by at most a relative w = 2^-22 + 2^-24 |t - max|: the fp32 product (t - max) log2e is off
by 2^-24 of itself, which exp2 turns into a relative |t - max| 2^-24 (log2e ln2 = 1); the hardware exp2, the reciprocal of the sum, the
sum's own roundings and the product with it are a few 2^-24 more, 2^-22 in all.  An element is firm when P's code at the reference's
block scale is the same for p (1 - w), p and p (1 + w); at most 1 % of a window is not.  Tolerance tier: e_kernel <= 2 e_chain, both
max |route - reference|, the bound of the integer core's tests.  Measured pairs: profiles/attention_mxf.txt."""
import pytest
import torch

from quantized_training import _native, fused, mx_attention, mx_operand
from quantized_training.fake_quantize import get_quantization_map
from test_gpu_attention_mxi import B, BF16, H, NEG, OPS, make_mask, randn3, routed

pytestmark = pytest.mark.gpu

NAMES = {"e4m3": "fp8_e4m3", "e5m2": "fp8_e5m2", "e2m1": "fp4_e2m1", "fp6": "fp6_e2m3"}
dev = torch.device("cuda:0")
QMAX = {"e4m3": 448.0, "e5m2": 57344.0, "e2m1": 6.0, "fp6": 7.5}


def qmap(fmt, dev="cpu"):
    return get_quantization_map(NAMES[fmt], dev)


def operands(q, k, v, fmt, dev, on_device=False, pow2=True, bs=32, dtype=BF16, fmt_v=None):
    """(qq, qs, kq, ks, vq, vs) of quantize_mx on `dev` (k^T as a view of the stored keys).  on_device: the packed operands it left are
    kept and read in place; else they are dropped (format and flag stay), so the route packs the values itself."""
    q, k, v = (t.to(dev, dtype) for t in (q, k, v))
    kT = k.transpose(-1, -2) if q.is_cuda else k.transpose(-1, -2).contiguous()
    sm = None if pow2 else qmap("e5m2", dev)
    (qs, qq), (ks, kq) = (OPS.quantize_mx(t, qmap(fmt, dev), [ax], bs, QMAX[fmt], pow2, sm, None) for t, ax in ((q, -1), (kT, -2)))
    vs, vq = OPS.quantize_mx(v, qmap(fmt_v or fmt, dev), [-2], bs, QMAX[fmt_v or fmt], pow2, sm, None)
    if not on_device:
        for t in (qq, kq, vq):
            mx_operand.drop_operand(t)
    return qq, qs, kq, ks, vq, vs


def reference(ops6, mask, scaling, is_div, fmt, parts=False):
    qq, qs, kq, ks, vq, vs = [t.cpu().double() for t in ops6]
    s = (qq * qs.repeat_interleave(32, -1)) @ (kq * ks.repeat_interleave(32, -2))
    s = s.float().to(BF16).float()
    s = (s / scaling if is_div else s * scaling).to(BF16)
    if mask is not None:
        s = (s.float() + mask.cpu().float()).to(BF16)
    p = torch.softmax(s.double(), -1)
    ps, pq = OPS.quantize_mx(p.to(BF16), qmap(fmt), [-1], 32, QMAX[fmt], True, None, None)
    out = ((pq.double() * ps.double().repeat_interleave(32, -1)) @ (vq * vs.repeat_interleave(32, -2))).float().to(BF16)
    return (out, s, p, ps, pq) if parts else out


def nodes(o, mask, scaling, fmt, pow2=True, bs=32):
    """Today's nodes, by hand."""
    dev = o[0].device
    s = OPS.matmul_mx(o[0], o[2], input_scale=o[1], weight_scale=o[3], block_size=bs) * scaling
    s = s if mask is None else s + mask
    ps, pq = OPS.quantize_mx(torch.softmax(s, -1), qmap(fmt, dev), [-1], bs, QMAX[fmt], pow2, None if pow2 else qmap("e5m2", dev), None)
    return OPS.matmul_mx(pq, o[4], input_scale=ps, weight_scale=o[5], block_size=bs)


def run(ops6, mask, scaling, is_div, fmt, native=True):
    with routed(native):
        out = OPS.attention_mx(*ops6, mask, scaling, is_div, qmap(fmt, ops6[0].device), QMAX[fmt], True, None, False, 32)
        Bq, Hq, Q, D = ops6[0].shape
        want = "qt_attention_mxf" if native else None                       # a switched-off call names no shape
        assert fused.routes_report().get(f"attention_mxf:{Bq}x{Hq}x{Q}x{ops6[2].shape[3]}x{D}") == want
    return out


CASES = [  # format, D, C, Q, mask, scaling applied as div, operands quantized on the device (their packed records are read in place)
    pytest.param("e4m3", 128, 128, 1, "none", False, True, id="e4m3-d128-c128-q1"),
    pytest.param("e4m3", 64, 384, 80, "causal", True, True, id="e4m3-d64-c384-q80-causal-div"),
    pytest.param("e5m2", 128, 256, 16, "padding", False, False, id="e5m2-d128-c256-q16-padding"),
    pytest.param("e5m2", 64, 128, 80, "causal", False, True, id="e5m2-d64-c128-q80-causal"),
    pytest.param("e2m1", 128, 384, 80, "causal", True, False, id="e2m1-d128-c384-q80-causal-div"),
    pytest.param("e2m1", 64, 256, 16, "padding", False, True, id="e2m1-d64-c256-q16-padding"),
    pytest.param("e2m1", 128, 128, 1, "none", False, True, id="e2m1-d128-c128-q1"),
]


@pytest.mark.parametrize("fmt,D,C,Q,kind,is_div,on_device", CASES)
def test_tolerance(fmt, D, C, Q, kind, is_div, on_device):
    ops6 = operands(*randn3(D, C, Q, 0), fmt, dev, on_device)
    assert (mx_operand.operand_record(ops6[2], mx_operand.SECOND) is not None) == on_device
    mask = make_mask(kind, Q, C, dev)
    scaling = D ** 0.5 if is_div else D ** -0.5
    ref = reference(ops6, mask, scaling, is_div, fmt).float()
    e_kernel = (run(ops6, mask, scaling, is_div, fmt).float().cpu() - ref).abs().max().item()
    e_chain = (run(ops6, mask, scaling, is_div, fmt, native=False).float().cpu() - ref).abs().max().item()
    print(f"attention_mxf {fmt} D {D} C {C} Q {Q} {kind} div {is_div}: e_kernel {e_kernel:.6g} e_chain {e_chain:.6g}")
    assert e_kernel <= 2 * e_chain, (e_kernel, e_chain)


@pytest.mark.parametrize("fmt,D,C,Q", [("e4m3", 64, 256, 80), ("e2m1", 128, 128, 16), ("e5m2", 128, 256, 16)])
def test_one_hot_and_uniform_rows(fmt, D, C, Q):
    q, k, v = randn3(D, C, Q, 1)
    v = torch.randint(-4, 5, v.shape, generator=torch.Generator().manual_seed(1)).to(BF16)     # every partial sum of P.V is exact in fp32
    ops6 = operands(q, k, v, fmt, dev)
    live = (torch.arange(B * H * Q) * 37 % C).view(B, H, Q)            # a different live key per row, over all key blocks
    hot = torch.full((B, H, Q, C), float("-inf"), dtype=BF16).scatter_(3, live[..., None], 0.0).to(dev)
    uniform = torch.full((B, 1, Q, C), NEG, dtype=BF16, device=dev)
    for mask in (hot, uniform):
        got, ref = run(ops6, mask, 0.125, False, fmt).cpu(), reference(ops6, mask, 0.125, False, fmt)
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    dead = hot.clone()
    dead[1, 2, Q - 1] = float("-inf")                                  # a row with no live key is NaN, and only that row
    got = run(ops6, dead, 0.125, False, fmt).cpu()
    assert got[1, 2, Q - 1].isnan().all() and not got[0].isnan().any() and not got[1, 2, :Q - 1].isnan().any()


@pytest.mark.parametrize("fmt,D,C,k0", [("e4m3", 64, 128, 32), ("e2m1", 128, 256, 96), ("e5m2", 128, 384, 200)])
def test_read_out(fmt, D, C, k0):
    g = torch.Generator().manual_seed(2)                              # integer q, k in [-2, 2]: every score is exact in fp32, so its
    q, k, v = (torch.randint(-2, 3, (B, H, n, D), generator=g).to(BF16) for n in (80, C, C))   # bf16 rounding is the reference's
    v.zero_()
    v[:, :, k0 + torch.arange(D), torch.arange(D)] = 1.0              # one 1 per column, at key k0 + d
    ops6 = operands(q, k, v, fmt, dev)
    ref, t, p, ps, pq = reference(ops6, None, D ** -0.5, False, fmt, parts=True)
    s, table = ps.float().repeat_interleave(32, -1), qmap(fmt)

    def code(y):                                                      # the element step at the reference's own block scale
        return table[(y.to(BF16).float() / s).to(BF16).view(torch.int16).long() & 0xFFFF]

    assert torch.equal(code(p), pq)
    w = 2.0 ** -22 + 2.0 ** -24 * (t.double() - t.double().amax(-1, keepdim=True)).abs()
    firm = ((code(p * (1 - w)) == pq) & (code(p * (1 + w)) == pq))[..., k0:k0 + D]
    print(f"read-out {fmt} D {D} C {C}: excused {(~firm).sum().item()} of {firm.numel()}")
    assert firm.float().mean().item() >= 0.99
    got = run(ops6, None, D ** -0.5, False, fmt).cpu()
    assert torch.equal(got.view(torch.int16)[firm], ref.view(torch.int16)[firm]), (got.float() - ref.float())[firm].abs().max()


def test_graph_replay_and_guard_margins():
    fmt, D, C, Q = "e4m3", 128, 384, 80
    ops6 = operands(*randn3(D, C, Q, 3), fmt, dev, on_device=True)
    mask = make_mask("causal", Q, C, dev)
    eager = run(ops6, mask, 0.125, False, fmt)
    packed = mx_attention.pack_operands_mxf(0, *ops6)
    n, pad = B * H * Q * D, 1024
    flat = torch.full((n + 2 * pad,), float("nan"), dtype=BF16, device=dev)
    out = flat[pad:pad + n].view(B, H, Q, D)
    args = (0, packed, mask, mask.stride()[:3], 0.125, False, qmap(fmt, dev), QMAX[fmt], out)
    _native.check(mx_attention.launch_mxf(*args), "qt_attention_mxf")  # warm-up: the LDS attribute is set outside the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _native.check(mx_attention.launch_mxf(*args), "qt_attention_mxf")
    for _ in range(2):
        out.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
        assert flat[:pad].isnan().all() and flat[pad + n:].isnan().all()


ARGS = "q eq k ek v ev mask msb msh msq scaling div fmt pmap qmax out B H Q C D bs stream".split()
BAD, OFF = -2, -3                                                               # QT_ERR_BAD_ARG, QT_ERR_UNALIGNED
REFUSALS = [({n: None}, BAD) for n in "q eq k ek v ev pmap out".split()]         # a pointer: None = NULL, a number = bytes off its slot
REFUSALS += [({n: v}, BAD) for n, v in [("B", -1), ("B", 70000), ("H", 0), ("Q", -1), ("C", 64), ("C", 192), ("C", 16512), ("D", 32), ("D", 96),
                                        ("bs", 64), ("fmt", 2), ("fmt", 3), ("fmt", 5), ("div", 2), ("scaling", float("nan")), ("qmax", 0.0),
                                        ("qmax", float("inf")), ("qmax", float("nan"))]]
REFUSALS += [({n: 8}, OFF) for n in "q k v".split()] + [({n: 2}, OFF) for n in ("ek", "ev")] + [
    (dict(out=4), OFF), (dict(pmap=1), OFF), (dict(mask=4), OFF), (dict(mask=0, msb=2), OFF), (dict(mask=0, msh=1), OFF), (dict(mask=0, msq=130), OFF)]


@pytest.mark.parametrize("change,code", [({}, 0)] + REFUSALS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_host_refusals(change, code):
    """Every refusal of the entry point, each returned before any launch (B 1, H 1, Q 16, C 128, D 64 on zeroed slots is taken)."""
    buf = torch.zeros(8 * 8192 + 131072, dtype=torch.uint8, device="cuda:0")
    slot = {n: buf.data_ptr() + 8192 * i for i, n in enumerate("q eq k ek v ev out mask pmap".split())}
    a = dict(slot, mask=None, msb=0, msh=0, msq=0, scaling=0.125, div=0, fmt=0, qmax=448.0, B=1, H=1, Q=16, C=128, D=64, bs=32, stream=None)
    for n, v in change.items():
        a[n] = (None if v is None else slot[n] + v) if n in slot else v
    assert _native.lib().qt_attention_mxf(*(a[n] for n in ARGS)) == code
    torch.cuda.synchronize()


FALLBACKS = [  # format of q / k, of v, block size, dtype, power-of-two scales, environment
    pytest.param("e4m3", "e5m2", 32, BF16, True, {}, id="mixed-formats"),
    pytest.param("fp6", "fp6", 32, BF16, True, {}, id="fp6"),
    pytest.param("e4m3", "e4m3", 32, BF16, False, {}, id="scales-not-pow2"),
    pytest.param("e4m3", "e4m3", 32, torch.float32, True, {}, id="fp32"),
    pytest.param("e4m3", "e4m3", 32, BF16, True, {"QT_FUSED_ATTENTION": "auto"}, id="rule-declines"),
    pytest.param("e2m1", "e2m1", 32, BF16, True, {"QT_MX_GEMM": "0"}, id="switched-off"),
]  # each bit-equal to the nodes run by hand and counted once (the switch forced on wherever it is not the case)


@pytest.mark.parametrize("fmt,fmt_v,bs,dtype,pow2,env", FALLBACKS)
def test_operator_fallbacks_are_the_nodes(fmt, fmt_v, bs, dtype, pow2, env, monkeypatch):
    monkeypatch.setattr(mx_attention, "_MXF_ATTENTION_TABLE", {})      # rule-declines: whatever the committed table lists
    o = operands(*randn3(64, 128, 16, 4), fmt, dev, True, pow2, bs, dtype, fmt_v)
    with routed(False, **(env or {"QT_FUSED_ATTENTION": "1"})):
        got = OPS.attention_mx(*o, None, 0.125, False, qmap(fmt, dev), QMAX[fmt], pow2, None if pow2 else qmap("e5m2", dev), False, bs)
        want = nodes(o, None, 0.125, fmt, pow2, bs)                    # under the same switches
    assert got.dtype == dtype and torch.equal(got, want)


def test_converted_toy_model_layer_by_layer():
    """convert_pt2e(fuse_attention=True) on the kernel route: each layer within the tolerance tier's bound of fuse_attention=False."""
    from test_attention_mxf_cpu import converted_toy
    x = torch.randn(1, 2, 128, 64, generator=torch.Generator().manual_seed(5)).to(BF16)
    mask = torch.zeros(1, 1, 128, 128, dtype=BF16).masked_fill(torch.ones(128, 128).triu(1).bool(), float("-inf"))
    plain, fused = (converted_toy(x.to(dev), mask.to(dev), fuse_attention=f).to(dev) for f in (False, True))
    with routed(True, n=2):
        got = fused(x.to(dev), mask.to(dev))
    want = plain(x.to(dev), mask.to(dev))
    for i in range(2):
        e = [(y[i].float().cpu() - reference(operands(*[x if i == 0 else y[0].cpu()] * 3, "e4m3", "cpu"), mask, 0.125, False, "e4m3").float())
             .abs().max().item() for y in (got, want)]
        print(f"toy layer {i}: e_kernel {e[0]:.6g} e_chain {e[1]:.6g}")
        assert e[0] <= 2 * e[1], (i, e)
