"""Chained converted int8 convolutions on the device: the codes-out entry points qt_q8_conv2d_codes, qt_q8_dwconv2d_codes and
qt_q8_gemm_codes (csrc/qt_mx_conv.hip, csrc/qt_mx_gemm.hip) through the C ABI, the operator quantized_ops.conv2d_qc with its fallbacks, the graph pass
fuse_conv_q_chains on converted blocks and their graph capture.

Every comparison is bit for bit: the new path adds no arithmetic whose order is free.  Exact tier: random int8 codes; the reference
is the host's (tests/conv_q_chain_cases.py: exact fp64 sums, the epilogue's rounding chain, torch.clamp, CPU quantize, narrowed), its
non-vacuity asserted on the expected side.  Everything else is compared with the parent's own chain on the device: the value entry
point or conv2d_q, torch's activation, the codes pass qt_quantize_codes_nhwc_*."""
import pytest
import torch
import torch.nn.functional as F

import conv_q_chain_cases as C
import conv_q_depthwise_cases as K
from conv_q_chain_cases import BF16, F32
from kernel_launch import nv, stream  # noqa: F401

pytestmark = pytest.mark.gpu
PAD = 256


class Margins:
    """A byte array on the device between two margins of `fill`."""

    def __init__(self, host, fill=0xFF):
        host = host.contiguous().view(torch.uint8).reshape(-1)
        self.n = host.numel()
        self.raw = torch.full((self.n + 2 * PAD,), fill, dtype=torch.uint8, device="cuda")
        self.raw[PAD:PAD + self.n] = host.cuda()
        self.image = self.raw.clone()
        assert self.ptr % 16 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + PAD

    def unchanged(self):
        return torch.equal(self.raw, self.image)


def ptr(t):
    return t.data_ptr() if t is not None else None


def launch_twice(call, count, operands, what):
    """call(y pointer) -> status, twice into 0x5A-filled buffers with margins: status 0, margins and operands intact, the same bytes."""
    runs = []
    for _ in range(2):
        buf = torch.full((count + 2 * PAD,), 0x5A, dtype=torch.uint8, device="cuda")
        rc = call(buf.data_ptr() + PAD)
        assert rc == 0, f"{what}: status {rc}"
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool((host[:PAD] == 0x5A).all()) and bool((host[PAD + count:] == 0x5A).all()), f"{what}: a margin of y was written"
        assert all(m.unchanged() for m in operands), f"{what}: an operand or its margins changed"
        runs.append(host[PAD:PAD + count].view(torch.int8))
    assert torch.equal(runs[0], runs[1]), f"{what}: two launches differ"
    return runs[0]


def same_codes(got, want, what):
    got, want = got.reshape(-1), want.reshape(-1)
    bad = got != want
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} codes differ, first at {int(bad.nonzero()[0])}: " \
                                f"{int(got[bad][0])} != {int(want[bad][0])}"


def entry_call(nv, family, key, xc, wc, dtype, bias, s, per_col, fold, tail, next_scale, qmap, codes=True):
    """y pointer -> status of the family's entry point (the codes sibling, or the value entry point with codes=False)."""
    L = nv.lib()
    head = lambda y: (xc.ptr, wc.ptr, y, int(dtype == F32), ptr(bias), ptr(s), per_col, fold)  # noqa: E731
    last = (*tail, ptr(next_scale), ptr(qmap), stream()) if codes else (stream(),)
    sfx = "_codes" if codes else ""
    if family == "gather":
        n, h, w = C.GATHER_M[key[0]]
        return lambda y: getattr(L, "qt_q8_conv2d" + sfx)(*head(y), n, h, w, 32, key[1], 3, 3, 2, 2, 1, 1, 1, 1, *last)
    if family == "dw":
        n, h, w, c, st = C.DW[key[0]]
        return lambda y: getattr(L, "qt_q8_dwconv2d" + sfx)(*head(y), n, h, w, c, 3, 3, st, st, 1, 1, 1, 1, *last)
    return lambda y: getattr(L, "qt_q8_gemm" + sfx)(*head(y), 1, C.GEMM_M, key[1], key[0], 0, 0, *last)


def exact_tier(nv, family, key, big=False):
    qmap = C.int8_map("cuda")
    ops = {"gather": C.gather_operands, "dw": C.dw_operands, "gemm": C.gemm_operands}[family](*key)
    xc, wc = Margins(ops["x"]), Margins(ops["w"])
    for dtype, per_channel, has_bias, act in C.settings(big):
        e = C.expectation(family, key, dtype, per_channel, has_bias, act)
        bias, s, ns = (e["bias"].cuda() if has_bias else None), e["s"].cuda(), e["next_scale"].cuda()
        call = entry_call(nv, family, key, xc, wc, dtype, bias, s, int(per_channel), e["fold"], C.tail_args(e["bounds"]), ns, qmap)
        what = f"{family} {key} {dtype} per_channel={per_channel} bias={has_bias} {act}"
        same_codes(launch_twice(call, e["codes"].numel(), (xc, wc), what), e["codes"], what)


@pytest.mark.parametrize("cout", C.GATHER_COUT)
@pytest.mark.parametrize("m", list(C.GATHER_M))
def test_gather_kernel_writes_the_expected_codes(nv, m, cout):
    """qt_q8_conv2d_codes, Cin = 32, 3 x 3, stride 2, padding 1: a ragged row tile (M = 126), a second tile of two rows (130); one
    run of columns, a partly empty 64-column half, a second column tile of one run; both model dtypes, scalar and per-channel
    factors, with and without bias, every activation setting."""
    exact_tier(nv, "gather", (m, cout))


@pytest.mark.parametrize("case", list(C.DW))
def test_depthwise_kernel_writes_the_expected_codes(nv, case):
    """qt_q8_dwconv2d_codes: one run, a ragged slab, a ragged second slab; stride 1 and 2; a problem on each side of the switch to
    two pixels per thread."""
    exact_tier(nv, "dw", (case,), big=case in C.DW_BIG)


@pytest.mark.parametrize("n", C.GEMM_N)
@pytest.mark.parametrize("k", C.GEMM_K)
def test_pointwise_gemm_writes_the_expected_codes(nv, k, n):
    """qt_q8_gemm_codes: K = 16 mod 32 (the contractions a pointwise layer brings), M = 130, one run of columns and a second tile."""
    exact_tier(nv, "gemm", (k, n))


def device_chain(nv, family, key, xc, wc, dtype, bias, s, per_col, fold, bounds, next_scale, qmap, rows, cout):
    """The parent's chain on the device: the value entry point, torch's activation, the codes pass -> int8 [rows, cout] on the host."""
    from quantized_training import pt2e_native
    y = torch.empty((rows, cout), dtype=dtype, device="cuda")
    assert entry_call(nv, family, key, xc, wc, dtype, bias, s, per_col, fold, None, None, None, codes=False)(y.data_ptr()) == 0
    t = y.view(1, rows, 1, cout).permute(0, 3, 1, 2)              # [1, C, rows, 1], channels_last-dense
    if bounds is not None:
        t = torch.relu(t) if bounds == (0.0, None) else F.hardtanh(t, bounds[0], bounds[1])
    codes = pt2e_native.conv_codes_nhwc(t, next_scale, qmap)
    assert codes is not None
    return codes.cpu()


@pytest.mark.parametrize("family,key", [("gather", (126, 48)), ("dw", ("c48_s2",)), ("gemm", (48, 16))])
def test_planted_specials_equal_the_device_chain(nv, family, key):
    """A NaN, a +inf and a -inf bias on single channels and a negative per-channel factor: the codes equal those of the parent's
    chain on the device; without an activation the NaN channel is code 0 and the infinities saturate."""
    qmap = C.int8_map("cuda")
    ops = {"gather": C.gather_operands, "dw": C.dw_operands, "gemm": C.gemm_operands}[family](*key)
    xc, wc = Margins(ops["x"]), Margins(ops["w"])
    rows, cout = ops["exact"].shape
    for dtype in (BF16, F32):
        for act in ("none", "relu", "hardtanh_0_6", "hardtanh_rounded_bounds"):
            bounds, sigma, next_scale = C.ACTS[act]
            bias, s = C.factors(cout, ops["k"], sigma, True, dtype, seed=5)
            bias[1], bias[2], bias[3] = float("nan"), float("inf"), float("-inf")
            s[5] = -s[5]
            bias, s, ns = bias.cuda(), s.cuda(), torch.tensor([next_scale]).to(dtype).cuda()
            what = f"{family} {key} {dtype} {act} with planted specials"
            call = entry_call(nv, family, key, xc, wc, dtype, bias, s, 1, 0, C.tail_args(bounds), ns, qmap)
            got = launch_twice(call, rows * cout, (xc, wc), what).view(rows, cout)
            same_codes(got, device_chain(nv, family, key, xc, wc, dtype, bias, s, 1, 0, bounds, ns, qmap, rows, cout), what)
            if act == "none":
                assert bool((got[:, 1] == 0).all()) and bool((got[:, 2] == 127).all()) and bool((got[:, 3] == -128).all())
            if act == "relu":
                assert bool((got[:, 1] == 0).all()) and bool((got[:, 2] == 127).all()) and bool((got[:, 3] == 0).all())


def test_entry_points_decline_before_any_launch(nv):
    """Cout = 24, a null map, a null scale, a misaligned y, act_lo > act_hi, a NaN bound and act = 2: the decline codes from all three
    entry points, and the output keeps its sentinel; an empty problem is status 0 without a launch."""
    L = nv.lib()
    x = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    w = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    y = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    ns, qmap = torch.ones(4, dtype=F32, device="cuda"), C.int8_map("cuda")
    nan = float("nan")

    def conv(cout=32, yp=y.data_ptr(), act=1, lo=0.0, hi=6.0, sp=ns.data_ptr(), mp=qmap.data_ptr(), n=1):
        return L.qt_q8_conv2d_codes(x.data_ptr(), w.data_ptr(), yp, 1, None, None, 0, 0, n, 4, 4, 32, cout, 1, 1, 1, 1, 0, 0, 1, 1,
                                    act, lo, hi, sp, mp, stream())

    def dwc(cout=32, yp=y.data_ptr(), act=1, lo=0.0, hi=6.0, sp=ns.data_ptr(), mp=qmap.data_ptr(), n=1):
        return L.qt_q8_dwconv2d_codes(x.data_ptr(), w.data_ptr(), yp, 1, None, None, 0, 0, n, 4, 4, cout, 1, 1, 1, 1, 0, 0, 1, 1,
                                      act, lo, hi, sp, mp, stream())

    def gemm(cout=32, yp=y.data_ptr(), act=1, lo=0.0, hi=6.0, sp=ns.data_ptr(), mp=qmap.data_ptr(), n=1):
        return L.qt_q8_gemm_codes(x.data_ptr(), w.data_ptr(), yp, 1, None, None, 0, 0, 1, 16 * n, cout, 16, 0, 0, act, lo, hi, sp, mp, stream())

    for call in (conv, dwc, gemm):
        assert call(cout=24) == nv.QT_ERR_BAD_ARG
        assert call(mp=None) == nv.QT_ERR_BAD_ARG and call(sp=None) == nv.QT_ERR_BAD_ARG
        assert call(lo=6.5) == nv.QT_ERR_BAD_ARG and call(lo=nan) == nv.QT_ERR_BAD_ARG and call(hi=nan) == nv.QT_ERR_BAD_ARG
        assert call(act=2) == nv.QT_ERR_BAD_ARG and call(act=-1) == nv.QT_ERR_BAD_ARG
        assert call(yp=y.data_ptr() + 8) == nv.QT_ERR_UNALIGNED and call(mp=qmap.data_ptr() + 1) == nv.QT_ERR_UNALIGNED
        assert call(sp=ns.data_ptr() + 2) == nv.QT_ERR_UNALIGNED
        assert call(n=0) == 0
        assert call(act=0, lo=7.0) == 0                            # the bounds are not read without an activation
        torch.cuda.synchronize()
        assert bool((y[512:] == 0x5A).all())                       # the one accepted call wrote its 16 x 32 codes and nothing else
    torch.cuda.synchronize()


# ---- the operator -----------------------------------------------------------------------------------------------------------------
ROUTES = {
    "gather": dict(cin=32, cout=48, k=(3, 3), groups=1, key="conv2d_int8"),
    "depthwise": dict(cin=48, cout=48, k=(3, 3), groups=48, key="conv2d_dw_int8"),
    "pointwise": dict(cin=48, cout=32, k=(1, 1), groups=1, key="conv2d_int8"),
}


def op_args(dtype, cin, cout, k, groups, n=2, h=9, w=7, per_channel=False, seed=0, device="cuda", **_):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, cin, h, w, generator=g) * 2).to(dtype).to(device)
    scale = torch.tensor(0.04).to(dtype).to(device)
    wc = torch.randint(-127, 128, (cout, *k, cin // groups), generator=g).to(torch.int8).to(device)
    b = torch.randint(-4000, 4000, (cout,), generator=g).to(dtype).to(device)
    kk = k[0] * k[1] * cin // groups
    base = 2.0 / (50 * 74 * kk ** 0.5)                            # codes of deviation 50 and 74: values of deviation about 2
    out_scale = (base * (0.5 + torch.rand(cout, 1, 1, generator=g)) if per_channel else torch.tensor([base])).to(dtype).to(device)
    padding = [0, 0] if k == (1, 1) else [1, 1]
    return x, scale, C.int8_map(device), wc, b, [1, 1], padding, [1, 1], groups, out_scale


def as_codes(x, scale, qmap):
    from quantized_training import pt2e_native
    n, c, h, w = x.shape
    return pt2e_native.conv_codes_nhwc(x, scale, qmap).view(n, h, w, c).permute(0, 3, 1, 2)


def parent_chain(x, scale, qmap, rest, bounds, next_scale, next_qmap):
    """conv2d_q, torch's activation, the consumer's quantize as int8 (the codes pass where it takes the tensor)."""
    from quantized_training import pt2e_native
    y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, *rest, None, "int8")
    if bounds is not None:
        y = torch.relu(y) if bounds == (0.0, None) else F.hardtanh(y, bounds[0], bounds[1])
    n, c, h, w = y.shape
    codes = pt2e_native.conv_codes_nhwc(y, next_scale, next_qmap) if y.is_cuda and c % 16 == 0 and y.dtype in (BF16, F32) else None
    if codes is not None:
        return codes.view(n, h, w, c).permute(0, 3, 1, 2)
    return C.narrow(torch.ops.quantized_ops.quantize(y, next_scale, None, None, None, next_qmap))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_operator_codes_in_and_codes_out(nv, monkeypatch, dtype, route):
    """On each route: conv2d_qc on the codes of an activation equals conv2d_q on its values; conv2d_qc with next_scale equals the
    parent chain, from values and from codes; the launches count in the kernel's key and in conv2d_codes_in / conv2d_codes_out."""
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    cfg = ROUTES[route]
    for per_channel, bounds in ((False, None), (True, (0.0, None)), (False, (0.0, 6.0)), (True, (-1.3, 1.1))):
        x, scale, qmap, *rest = op_args(dtype, per_channel=per_channel, **cfg)
        ns = torch.tensor(0.02).to(dtype).cuda()
        lo, hi = bounds if bounds is not None else (None, None)
        want_y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, *rest, None, "int8")
        want_c = parent_chain(x, scale, qmap, rest, bounds, ns, qmap)
        codes = as_codes(x, scale, qmap)
        before, reasons = dict(pt2e_native.STATS), dict(pt2e_native.CONV_Q_REASONS)
        y = torch.ops.quantized_ops.conv2d_qc(codes, None, None, *rest, None, "int8", None, None, None, None)
        c1 = torch.ops.quantized_ops.conv2d_qc(x, scale, qmap, *rest, None, "int8", lo, hi, ns, qmap)
        c2 = torch.ops.quantized_ops.conv2d_qc(codes, None, None, *rest, None, "int8", lo, hi, ns, qmap)
        ran = {k: pt2e_native.STATS[k] - before[k] for k in before if pt2e_native.STATS[k] != before[k]}
        assert ran == {cfg["key"]: 3, "conv2d_codes_in": 2, "conv2d_codes_out": 2}, ran
        assert pt2e_native.CONV_Q_REASONS == reasons
        assert y.dtype == dtype and y.shape == want_y.shape and y.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(y.view(torch.int16 if dtype == BF16 else torch.int32), want_y.view(torch.int16 if dtype == BF16 else torch.int32))
        for c in (c1, c2):
            assert c.dtype == torch.int8 and c.shape == want_y.shape and c.is_contiguous(memory_format=torch.channels_last)
            same_codes(c.cpu(), want_c.cpu(), f"conv2d_qc {route} {dtype} {bounds}")
        assert want_c.unique().numel() >= 32


FALLBACKS = {
    "route_rule": dict(route="gather", rule=True),
    "dw_route_rule": dict(route="depthwise", rule=True),
    "fp16": dict(route="gather", dtype=torch.float16),
    "cout_24": dict(route="pointwise", cout=24),
}


@pytest.mark.parametrize("which", list(FALLBACKS))
def test_operator_fallbacks_give_the_same_bits(nv, monkeypatch, which):
    """A route rule, fp16, Cout = 24: conv2d_qc runs the graph's own nodes -- the same codes as the parent chain, the same values
    from a code array as conv2d_q from the values -- and each call counts one reason."""
    from quantized_training import pt2e_native
    cfg = dict(FALLBACKS[which])
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", cfg.pop("rule", False))
    dtype = cfg.pop("dtype", BF16)
    shape = dict(ROUTES[cfg.pop("route")])
    shape.update(cfg)
    x, scale, qmap, *rest = op_args(dtype, **shape)
    ns, bounds = torch.tensor(0.02).to(dtype).cuda(), (0.0, 6.0)
    want_y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, *rest, None, "int8")
    want_c = parent_chain(x, scale, qmap, rest, bounds, ns, qmap)
    codes = C.narrow(torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap)).contiguous(memory_format=torch.channels_last)

    def reasons():
        return sum(pt2e_native.CONV_Q_REASONS.values())
    native_values = which == "cout_24"                      # the values come from the kernel; only the codes-out half falls back
    before, r0 = dict(pt2e_native.STATS), reasons()
    c1 = torch.ops.quantized_ops.conv2d_qc(x, scale, qmap, *rest, None, "int8", *bounds, ns, qmap)
    assert reasons() == r0 + 1
    c2 = torch.ops.quantized_ops.conv2d_qc(codes, None, None, *rest, None, "int8", *bounds, ns, qmap)
    assert reasons() == r0 + 2
    y = torch.ops.quantized_ops.conv2d_qc(codes, None, None, *rest, None, "int8", None, None, None, None)
    assert reasons() == r0 + (2 if native_values else 3)
    assert pt2e_native.STATS["conv2d_codes_out"] == before["conv2d_codes_out"]
    assert pt2e_native.STATS["conv2d_codes_in"] - before["conv2d_codes_in"] == (2 if native_values else 0)
    assert y.dtype == dtype and torch.equal(y.view(torch.int16), want_y.view(torch.int16))
    for c in (c1, c2):
        assert c.dtype == torch.int8 and c.shape == want_y.shape
        same_codes(c.cpu(), want_c.cpu(), f"fallback {which}")


def test_operator_runs_on_cpu_tensors(nv):
    """Host tensors: codes in and codes out through the graph's own nodes; the device's codes for the same call are the same."""
    cfg = ROUTES["depthwise"]
    x, scale, qmap, *rest = op_args(BF16, device="cpu", **cfg)
    ns = torch.tensor(0.02).to(BF16)
    codes = C.narrow(torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap)).contiguous(memory_format=torch.channels_last)
    want = parent_chain(x, scale, qmap, rest, (0.0, 6.0), ns, qmap)
    got = torch.ops.quantized_ops.conv2d_qc(codes, None, None, *rest, None, "int8", 0.0, 6.0, ns, qmap)
    assert got.dtype == torch.int8 and torch.equal(got, want)
    y = torch.ops.quantized_ops.conv2d_qc(codes, None, None, *rest, None, "int8", None, None, None, None)
    assert torch.equal(y, torch.ops.quantized_ops.conv2d_q(x, scale, qmap, *rest, None, "int8"))


# ---- converted graphs -------------------------------------------------------------------------------------------------------------
def chained_and_plain(net_cls, monkeypatch):
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    monkeypatch.setenv("QT_PT2E_NATIVE", "1")
    plain, x = K.convert_block(BF16, device="cuda", native=None, net=C.seeded(net_cls))
    chained, _ = K.convert_block(BF16, device="cuda", native=None, net=C.seeded(net_cls))
    assert C.call_targets(chained) == C.call_targets(plain)
    return plain, chained, x


@pytest.mark.parametrize("net_cls,act", [(K.Block, "aten.relu.default"), (C.Block6, "aten.hardtanh.default")], ids=["relu", "relu6"])
def test_converted_block_chains_its_convolutions(nv, monkeypatch, net_cls, act):
    """expand -> act -> depthwise -> act -> project: two edges rewritten, the two activation nodes between them gone, three conv2d_qc
    nodes; the output equals the un-chained native graph's bit for bit; two codes-out and two codes-in launches, no fallback; a
    torch.cuda.graph replay equals the eager call."""
    from quantized_training import pt2e_native
    plain, chained, x = chained_and_plain(net_cls, monkeypatch)
    assert C.call_targets(plain).count(act) == 3
    assert pt2e_native.fuse_conv_q_chains(chained) == 2 and pt2e_native.fuse_conv_q_chains(chained) == 0
    t = C.call_targets(chained)
    assert t.count("quantized_ops.conv2d_qc.default") == 3 and t.count("quantized_ops.conv2d_q.default") == 0 and t.count(act) == 1
    with torch.no_grad():
        want = plain(x)
        before, reasons = dict(pt2e_native.STATS), dict(pt2e_native.CONV_Q_REASONS)
        got = chained(x).clone()
    ran = {k: pt2e_native.STATS[k] - before[k] for k in before if pt2e_native.STATS[k] != before[k]}
    assert ran == {"conv2d_int8": 2, "conv2d_dw_int8": 1, "conv2d_codes_in": 2, "conv2d_codes_out": 2}, ran
    assert pt2e_native.CONV_Q_REASONS == reasons
    assert got.dtype == want.dtype and torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert bool(got.float().isfinite().all()) and got.float().unique().numel() > 32

    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        chained(static_x)                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = chained(static_x)
    assert pt2e_native.CONV_Q_REASONS == reasons
    static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), got.view(torch.int16))


def test_convert_pt2e_chain_convs_switch(nv, monkeypatch):
    """convert_pt2e(chain_convs=True) on the device applies the pass behind the native passes; the default leaves today's graph."""
    from quantized_training import pt2e_native, quantize_pt2e as qp
    plain, _, x = chained_and_plain(K.Block, monkeypatch)
    net = C.seeded(K.Block).cuda().to(BF16).eval()
    gm = qp.prepare_pt2e(net, qp.get_default_quantizer(K.SPEC, None, K.SPEC, "int24"), (x,))
    with torch.no_grad():
        gm(x), gm(x * 0.5)
    chained = qp.convert_pt2e(gm, chain_convs=True)
    assert C.call_targets(chained).count("quantized_ops.conv2d_qc.default") == 3
    assert C.call_targets(plain).count("quantized_ops.conv2d_q.default") == 3
    with torch.no_grad():
        assert torch.equal(chained(x).view(torch.int16), plain(x).view(torch.int16))
