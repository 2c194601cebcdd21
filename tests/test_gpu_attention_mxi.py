"""The block-scaled integer attention core (qt_attention_mxi) and its operator attention_mx against the six-step chain of the nodes it
replaces (csrc/qt_attention_mxi.hip's header), evaluated on the CPU with sums and the softmax in float64 and the stated roundings.
Exact tier, bit for bit: one-hot rows, uniform rows, and the read-out (V an identity window, the output is P' there) wherever the
reference's own p is not within one fp32 ulp (a relative 2^-23, the step of the kernel's fp32 exponential) of a point at which its code
map(bf16(bf16(p) / s)) changes, s being the reference's block scale; on the CPU under 0.01 % of either window is so excused.
Tolerance tier: e_kernel = max |kernel - reference| <= 2 e_chain = 2 max |today's nodes on the device - reference| per case (both routes
may flip different P codes at rounding boundaries and round the exponential elsewhere).  Measured pairs: profiles/attention_mxi.txt."""
import contextlib
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NEG = float(torch.finfo(BF16).min)
B, H = 2, 3
OPS = torch.ops.quantized_ops


def maps(dev="cpu"):
    from quantized_training.fake_quantize import get_quantization_map
    return get_quantization_map("int6", dev), get_quantization_map("fp8_e5m3", dev)


def randn3(D, C, Q, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, H, n, D, generator=g).to(BF16) for n in (Q, C, C)]


def operands(q, k, v, pow2, dev="cpu", bs=64, dtype=BF16):
    """q, k, v through the CPU quantize_mx (int6): (qq, qs, kq, ks, vq, vs) on `dev`, their integer records along."""
    from quantized_training import mx_operand
    qm, sm = maps()
    a = (qm, [-1], bs, 31.0, pow2, None if pow2 else sm, None)
    b = (qm, [-2], bs, 31.0, pow2, None if pow2 else sm, None)
    (qs, qq), (ks, kq), (vs, vq) = (OPS.quantize_mx(q.to(dtype), *a), OPS.quantize_mx(k.to(dtype).transpose(-1, -2).contiguous(), *b),
                                    OPS.quantize_mx(v.to(dtype), *b))
    return [mx_operand.copy_hints(t, t.to(dev)) for t in (qq, qs, kq, ks, vq, vs)]


def block_matmul(a, sa, b, sb):
    """a [.., M, K] with scales [.., M, K/64]; b [.., K, N] with scales [.., K/64, N] -> fp32 chain over the blocks, bf16."""
    acc = torch.zeros(a.shape[:-1] + (b.shape[-1],), dtype=torch.float32)
    for kb in range(a.shape[-1] // 64):
        p = a[..., kb * 64:(kb + 1) * 64].double() @ b[..., kb * 64:(kb + 1) * 64, :].double()
        acc = (p * (sa[..., kb:kb + 1].float() * sb[..., kb:kb + 1, :].float()).double() + acc.double()).float()
    return acc.to(BF16)


def reference(ops6, mask, scaling, is_div, pow2, parts=False):
    qq, qs, kq, ks, vq, vs = [t.cpu() for t in ops6]
    qm, sm = maps()
    s = block_matmul(qq, qs, kq, ks).float()
    s = (s / scaling if is_div else s * scaling).to(BF16)
    if mask is not None:
        s = (s.float() + mask.cpu().float()).to(BF16)
    p = torch.softmax(s.double(), -1)
    ps, pq = OPS.quantize_mx(p.to(BF16), qm, [-1], 64, 31.0, pow2, None if pow2 else sm, None)
    out = block_matmul(pq, ps, vq, vs)
    return (out, p, ps, pq) if parts else out


def nodes(o, mask, scaling, pow2, bs=64):
    """Today's nodes, by hand."""
    qm, sm = maps(o[0].device)
    s = OPS.matmul_mx(o[0], o[2], input_scale=o[1], weight_scale=o[3], block_size=bs) * scaling
    s = s if mask is None else s + mask
    ps, pq = OPS.quantize_mx(torch.softmax(s, -1), qm, [-1], bs, 31.0, pow2, None if pow2 else sm, None)
    return OPS.matmul_mx(pq, o[4], input_scale=ps, weight_scale=o[5], block_size=bs)


def make_mask(kind, Q, C, dev):
    if kind == "none":
        return None
    if kind == "causal":                   # -inf above the diagonal that ends in the last key; per (b, h, q), row stride C + 8
        keep = torch.arange(C)[None, :] <= torch.arange(Q)[:, None] + (C - Q)
        m = torch.full((B, H, Q, C + 8), 1.0, dtype=BF16)
        m[..., :C] = torch.where(keep, 0.0, float("-inf")).to(BF16)
        return m.to(dev)[..., :C]
    pad = torch.zeros(B, 1, 1, C, dtype=BF16)  # padding: the last keys of batch b at the bf16 minimum, broadcast over heads and rows
    for b in range(B):
        pad[b, 0, 0, C - 5 - 9 * b:] = NEG
    return pad.to(dev)


@contextlib.contextmanager
def routed(native, n=1, **env):
    """QT_FUSED_ATTENTION forced on (or off / `env`); on leaving, `n` more calls counted on that route and the report left as found."""
    from quantized_training import mx_attention
    env = env if env or native is None else {"QT_FUSED_ATTENTION": "1" if native else "0"}
    os.environ.update(env)
    key = "attention_native" if native else "attention_fallback"
    before = mx_attention.STATS[key]
    try:
        yield
        assert mx_attention.STATS[key] == before + n, (key, mx_attention.STATS, before)
    finally:
        for k in env:
            del os.environ[k]
        mx_attention.ATTENTION_MXI_ROUTES.clear()


def run(ops6, mask, scaling, is_div, pow2, native=True, bs=64):
    from quantized_training import fused
    qm, sm = maps(ops6[0].device)
    with routed(native):
        out = OPS.attention_mx(*ops6, mask, scaling, is_div, qm, 31.0, pow2, None if pow2 else sm, False, bs)
        Bq, Hq, Q, D = ops6[0].shape
        want = "qt_attention_mxi" if native else None                       # a switched-off call names no shape
        assert fused.routes_report().get(f"attention_mxi:{Bq}x{Hq}x{Q}x{ops6[2].shape[3]}x{D}") == want
    return out


CASES = [  # D, C, Q, mask, power-of-two scales, scaling applied as div
    pytest.param(64, 64, 1, "none", False, False, id="d64-c64-q1"),
    pytest.param(128, 128, 16, "causal", False, True, id="d128-c128-q16-causal-div"),
    pytest.param(128, 192, 80, "padding", True, False, id="d128-c192-q80-padding-pow2"),
    pytest.param(64, 192, 80, "causal", False, False, id="d64-c192-q80-causal"),
    pytest.param(128, 64, 16, "none", True, True, id="d128-c64-q16-pow2-div"),
]


@pytest.mark.parametrize("D,C,Q,kind,pow2,is_div", CASES)
def test_tolerance(D, C, Q, kind, pow2, is_div):
    dev = torch.device("cuda:0")
    ops6 = operands(*randn3(D, C, Q, 0), pow2, dev)
    mask = make_mask(kind, Q, C, dev)
    scaling = D ** 0.5 if is_div else D ** -0.5
    ref = reference(ops6, mask, scaling, is_div, pow2).float()
    e_kernel = (run(ops6, mask, scaling, is_div, pow2).float().cpu() - ref).abs().max().item()
    e_chain = (run(ops6, mask, scaling, is_div, pow2, native=False).float().cpu() - ref).abs().max().item()
    print(f"attention_mxi D {D} C {C} Q {Q} {kind} pow2 {pow2} div {is_div}: e_kernel {e_kernel:.6g} e_chain {e_chain:.6g}")
    assert e_kernel <= 2 * e_chain, (e_kernel, e_chain)


@pytest.mark.parametrize("D,C,Q,pow2", [(64, 192, 80, False), (128, 128, 16, True)])
def test_one_hot_and_uniform_rows(D, C, Q, pow2):
    dev = torch.device("cuda:0")
    ops6 = operands(*randn3(D, C, Q, 1), pow2, dev)
    live = (torch.arange(B * H * Q) * 37 % C).view(B, H, Q)            # a different live key per row, over all key blocks
    hot = torch.full((B, H, Q, C), float("-inf"), dtype=BF16).scatter_(3, live[..., None], 0.0).to(dev)
    uniform = torch.full((B, 1, Q, C), NEG, dtype=BF16, device=dev)
    for mask in (hot, uniform):
        got, ref = run(ops6, mask, 0.125, False, pow2).cpu(), reference(ops6, mask, 0.125, False, pow2)
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    dead = hot.clone()
    dead[1, 2, Q - 1] = float("-inf")                                  # a row with no live key is NaN, and only that row
    got = run(ops6, dead, 0.125, False, pow2).cpu()
    assert got[1, 2, Q - 1].isnan().all() and not got[0].isnan().any() and not got[1, 2, :Q - 1].isnan().any()


@pytest.mark.parametrize("D,C,k0", [(64, 128, 32), (128, 192, 64)])
def test_read_out(D, C, k0):
    dev = torch.device("cuda:0")
    q, k, v = randn3(D, C, 80, 2)
    v.zero_()
    v[:, :, k0 + torch.arange(D), torch.arange(D)] = 1.0              # one 1 per column, at key k0 + d
    ops6 = operands(q, k, v, False, dev)
    ref, p, ps, pq = reference(ops6, None, D ** -0.5, False, False, parts=True)
    s = ps.float().repeat_interleave(64, -1)

    def code(y):                                                      # the element step at the reference's own block scale
        return (y.to(BF16).float() / s).to(BF16).float().round().clamp(-32, 31)

    assert torch.equal(code(p), pq.float())
    firm = ((code(p * (1 - 2.0 ** -23)) == pq.float()) & (code(p * (1 + 2.0 ** -23)) == pq.float()))[..., k0:k0 + D]
    print(f"read-out D {D} C {C}: excused {(~firm).sum().item()} of {firm.numel()}")
    assert firm.float().mean().item() > 0.5
    got = run(ops6, None, D ** -0.5, False, False).cpu()
    assert torch.equal(got.view(torch.int16)[firm], ref.view(torch.int16)[firm]), (got.float() - ref.float())[firm].abs().max()


def test_graph_replay_and_guard_margins():
    from quantized_training import _native, mx_attention
    dev = torch.device("cuda:0")
    D, C, Q = 128, 192, 80
    ops6 = operands(*randn3(D, C, Q, 3), False, dev)
    mask = make_mask("causal", Q, C, dev)
    eager = run(ops6, mask, 0.125, False, False)
    packed = mx_attention.pack_operands(*ops6)
    n, pad = B * H * Q * D, 1024
    flat = torch.full((n + 2 * pad,), float("nan"), dtype=BF16, device=dev)
    out = flat[pad:pad + n].view(B, H, Q, D)
    args = (packed, mask, mask.stride()[:3], 0.125, False, "int6", 31.0, False, maps(dev)[1], out)
    _native.check(mx_attention.launch(*args), "qt_attention_mxi")     # warm-up: the LDS attribute is set outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _native.check(mx_attention.launch(*args), "qt_attention_mxi")
    for _ in range(2):
        out.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
        assert flat[:pad].isnan().all() and flat[pad + n:].isnan().all()


ARGS = "q sq k sk v sv vw svw mask msb msh msq scaling div fmt qmax pow2 smap out B H Q C D bs stream".split()
BAD, OFF = -2, -3                                                               # QT_ERR_BAD_ARG, QT_ERR_UNALIGNED
REFUSALS = [({n: None}, BAD) for n in "q sq k sk v sv vw svw out fmt".split()]   # a pointer: None = NULL, a number = bytes off its slot
REFUSALS += [({n: v}, BAD) for n, v in [("B", -1), ("B", 70000), ("H", 0), ("Q", -1), ("Q", 65535 * 64 + 1), ("C", 32), ("C", 96), ("C", 16448),
                                        ("D", 32), ("bs", 32), ("div", 2), ("scaling", float("nan")), ("qmax", 0.0), ("qmax", float("inf")),
                                        ("qmax", float("nan")), ("kind", "fp8_e4m3"), ("flo", -129.0), ("fhi", 128.0), ("flo", -31.5),
                                        ("fhi", 30.5), ("flo", 32.0)]] + [(dict(pow2=1, smap=0), BAD)]
REFUSALS += [({n: 8}, OFF) for n in "q k v vw sk svw".split()] + [({n: 2}, OFF) for n in ("sq", "sv")] + [
    (dict(out=4), OFF), (dict(smap=1), OFF), (dict(mask=4), OFF), (dict(mask=0, msb=2), OFF), (dict(mask=0, msh=1), OFF), (dict(mask=0, msq=66), OFF)]


@pytest.mark.parametrize("change,code", [({}, 0)] + REFUSALS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_host_refusals(change, code):
    """Every refusal of the entry point, each returned before any launch (B 1, H 1, Q 16, C 64, D 64 on zeroed 4 KiB slots is taken)."""
    from quantized_training import _native
    buf = torch.zeros(12 * 4096, dtype=torch.uint8, device="cuda:0")
    slot = {n: buf.data_ptr() + 4096 * i for i, n in enumerate("q sq k sk v sv vw svw out mask smap".split())}
    fmt = _native.format_for(change.get("kind", "int6"))
    fmt.flo, fmt.fhi = change.get("flo", fmt.flo), change.get("fhi", fmt.fhi)
    a = dict(slot, mask=None, smap=None, msb=0, msh=0, msq=0, scaling=0.125, div=0, fmt=ctypes.byref(fmt), qmax=31.0, pow2=0, B=1, H=1, Q=16, C=64,
             D=64, bs=64, stream=None)
    for n, v in change.items():
        if n in slot:
            a[n] = None if v is None else slot[n] + v
        elif n in a:
            a[n] = v
    assert _native.lib().qt_attention_mxi(*(a[n] for n in ARGS)) == code
    torch.cuda.synchronize()


FALLBACKS = [  # D, block size, dtype, operands keep their record, environment
    pytest.param(64, 64, BF16, True, {"QT_MX_GEMM": "0"}, id="switched-off"),
    pytest.param(64, 64, BF16, True, {"QT_FUSED_ATTENTION": "auto"}, id="rule-declines"),
    pytest.param(64, 64, BF16, False, {}, id="no-record"),
    pytest.param(64, 64, torch.float32, True, {}, id="fp32"),
    pytest.param(64, 64, torch.float16, True, {}, id="fp16"),
    pytest.param(64, 32, BF16, True, {}, id="block-32"),
    pytest.param(192, 64, BF16, True, {}, id="head-dim-192"),
]


@pytest.mark.parametrize("D,bs,dtype,record,env", FALLBACKS)
def test_operator_fallbacks_are_the_nodes(D, bs, dtype, record, env):
    """Each fallback is bit-equal to the nodes run by hand (forced wherever the switch is not the case); the native route is counted in run()."""
    dev = torch.device("cuda:0")
    qm, sm = maps(dev)
    o = operands(*randn3(D, 128, 16, 4), False, dev, bs, dtype)
    o = o if record else [t.clone() for t in o]                                # clones carry no record
    with routed(False, **(env or {"QT_FUSED_ATTENTION": "1"})):
        got = OPS.attention_mx(*o, None, 0.125, False, qm, 31.0, False, sm, False, bs)
        want = nodes(o, None, 0.125, False, bs)                                # under the same switches
    assert got.dtype == dtype and torch.equal(got, want)


def test_converted_toy_model_layer_by_layer():
    """convert_pt2e(fuse_attention=True) on the device, kernel route: each layer within the tolerance tier's bound of fuse_attention=False,
    either graph's layer against the reference chain on that graph's own layer input."""
    from test_attention_mxi_cpu import converted_toy
    dev = torch.device("cuda:0")
    x = randn3(64, 128, 128, 5)[0]
    mask = torch.zeros(1, 1, 128, 128, dtype=BF16).masked_fill(torch.ones(128, 128).triu(1).bool(), float("-inf"))
    plain, fused = (converted_toy(x.to(dev), mask.to(dev), fuse_attention=f).to(dev) for f in (False, True))
    with routed(True, n=2):
        got = fused(x.to(dev), mask.to(dev))
    want = plain(x.to(dev), mask.to(dev))
    for i in range(2):
        e = [(y[i].float().cpu() - reference(operands(*[x if i == 0 else y[0].cpu()] * 3, False), mask, 0.125, False, False).float()).abs().max().item()
             for y in (got, want)]
        print(f"toy layer {i}: e_kernel {e[0]:.6g} e_chain {e[1]:.6g}")
        assert e[0] <= 2 * e[1], (i, e)
