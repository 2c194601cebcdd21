"""The split of K of the native int8 convolution on the device: qt_q8_conv2d_ws / qt_q8_conv2d_codes_ws (csrc/qt_mx_conv.hip) through
the C ABI, the operator conv2d_q on a layer the pass marked (convert_pt2e(split_k=True)), a converted CNN with a projecting 1 x 1
layer, its graph capture and its chained form.

Exact tier: int32 partial sums add exactly in any order, so every forced split must give, bit for bit, (a) the host's rounding chain
on the exact fp64 sums and (b) what the unsplit qt_q8_conv2d writes for the same operands.  The output sits between NaN margins, the
workspace and the tickets between margins of 0xFF; two launches into one workspace give the same bits (the ticket reset works) and
every ticket is zero afterwards."""
import pytest
import torch

import conv_q_splitk_cases as C
from conv_q_splitk_cases import BF16, F32, SLAB
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

    def body(self):
        return self.raw[PAD:PAD + self.n]

    def margins_intact(self):
        return torch.equal(self.raw[:PAD], self.image[:PAD]) and torch.equal(self.raw[PAD + self.n:], self.image[PAD + self.n:])

    def unchanged(self):
        return torch.equal(self.raw, self.image)


class Scratch:
    """A workspace of `tiles * splits` slabs and `tiles` tickets, each between margins of 0xFF; the tickets start at zero, the
    workspace at 0xFF (a partial sum that was never written would read as -1 everywhere)."""

    def __init__(self, tiles, splits):
        self.ws = Margins(torch.full((tiles * splits * SLAB,), 0xFF, dtype=torch.uint8))
        self.tickets = Margins(torch.zeros(tiles * 4, dtype=torch.uint8))
        self.n_tickets = tiles

    def args(self, ksplit):
        return ksplit, self.ws.ptr, self.ws.n, self.tickets.ptr, self.n_tickets

    def check(self, what):
        assert self.ws.margins_intact(), f"{what}: a margin of the workspace was written"
        assert self.tickets.margins_intact(), f"{what}: a margin of the tickets was written"
        assert not bool(self.tickets.body().any()), f"{what}: a ticket is not zero after the launch"


def ptr(t):
    return t.data_ptr() if t is not None else None


def geo_args(case):
    n, h, w, cin, cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw) = C.CASES[case][0]
    return n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw


def out_count(case):
    ho, wo = C.geometry(case)
    return C.CASES[case][0][0] * ho * wo, C.CASES[case][0][4]


def launch(nv, case, xc, wc, dtype, bias, s, per_col, fold, scratch=None, ksplit=1, launches=1):
    """The value entry points into NaN-filled buffers: status 0, margins and operands intact, every launch the same bits -> y [M, Cout]
    on the host.  scratch None: the unsplit qt_q8_conv2d."""
    rows, cout = out_count(case)
    count, pad = rows * cout, 64
    what = f"{case} S={ksplit} {dtype}"
    b = bias.to(dtype).cuda() if bias is not None else None
    sd = s.to(dtype).cuda() if s is not None else None
    runs = []
    for _ in range(launches):
        buf = torch.full((count + 2 * pad,), float("nan"), dtype=dtype, device="cuda")
        head = (xc.ptr, wc.ptr, buf.data_ptr() + pad * buf.element_size(), int(dtype == F32), ptr(b), ptr(sd), per_col, fold, *geo_args(case))
        if scratch is None:
            rc = nv.lib().qt_q8_conv2d(*head, stream())
        else:
            rc = nv.lib().qt_q8_conv2d_ws(*head, *scratch.args(ksplit), stream())
        assert rc == 0, f"{what}: status {rc}"
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool(host[:pad].isnan().all()) and bool(host[pad + count:].isnan().all()), f"{what}: a margin of y was written"
        assert xc.unchanged() and wc.unchanged(), f"{what}: an operand or its margins changed"
        if scratch is not None:
            scratch.check(what)
        runs.append(host[pad:pad + count].reshape(rows, cout))
    bits = torch.int16 if dtype == BF16 else torch.int32
    for other in runs[1:]:
        assert torch.equal(runs[0].view(bits), other.view(bits)), f"{what}: two launches differ"
    assert not bool(runs[0].isnan().any()), f"{what}: an element of y was not written (or a margin was read)"
    return runs[0]


def same_bits(got, want, what):
    bits = torch.int16 if got.dtype == BF16 else torch.int32
    got, want = got.reshape(-1), want.reshape(-1)
    bad = got.contiguous().view(bits) != want.contiguous().view(bits)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {int(bad.nonzero()[0])}: " \
                                f"{got[bad][0].item()} != {want[bad][0].item()}"


SPLITS = [(case, s) for case, (_, forced) in C.CASES.items() for s in forced]


@pytest.mark.parametrize("case,ksplit", SPLITS, ids=[f"{c}-S{s}" for c, s in SPLITS])
def test_forced_split_is_exact(nv, case, ksplit):
    """Every forced split of every case: the bare fp32 sums and the bf16 output with bias and per-channel factors equal the host
    chain and the unsplit kernel bit for bit; two launches into one workspace agree and leave the tickets zero."""
    ops = C.operands(case)
    exact, bias, scale = ops["exact"], ops["bias"], ops["scale"]
    tiles, nk = C.tiles_nk(case)
    assert 1 < ksplit <= nk
    if case == "pm127_odd":
        assert float(exact.abs().max()) > 2 ** 24 and bool((exact.float().double() != exact).any())      # the conversion does round
    if case == "m128_longest":
        assert float(exact.max()) == ((1 << 17) - 32) * 16384 < 2 ** 31
    xc, wc = Margins(ops["x"]), Margins(ops["w"])
    scratch = Scratch(tiles, ksplit)
    rows = exact.reshape(-1, exact.shape[-1])
    got = launch(nv, case, xc, wc, F32, None, None, 0, 0, scratch, ksplit, launches=2)
    same_bits(got, C.chain(rows, None, None, F32, 0), f"{case} S={ksplit} bare fp32 against the host chain")
    same_bits(got, launch(nv, case, xc, wc, F32, None, None, 0, 0), f"{case} S={ksplit} bare fp32 against the unsplit kernel")
    b16, s16 = bias.bfloat16(), scale.bfloat16()
    got = launch(nv, case, xc, wc, BF16, b16, s16, 1, 0, scratch, ksplit, launches=2)
    same_bits(got, C.chain(rows, b16, s16, BF16, 0), f"{case} S={ksplit} bf16 against the host chain")
    same_bits(got, launch(nv, case, xc, wc, BF16, b16, s16, 1, 0), f"{case} S={ksplit} bf16 against the unsplit kernel")


def test_epilogue_variants_under_a_split(nv):
    """One case (Cin = 96, stride 2, S = 4): bf16 and fp32, bias, per-tensor and per-channel factor, the fp32 fold on and off."""
    case, ksplit = "mid_pixel_stride", 4
    ops = C.operands(case)
    rows, bias, scale = ops["exact"].reshape(-1, ops["exact"].shape[-1]), ops["bias"], ops["scale"]
    xc, wc = Margins(ops["x"]), Margins(ops["w"])
    scratch = Scratch(C.tiles_nk(case)[0], ksplit)
    same_bits(launch(nv, case, xc, wc, BF16, None, None, 0, 0, scratch, ksplit), C.chain(rows, None, None, BF16, 0), "bare bf16")
    for per_col in (0, 1):
        s = scale if per_col else scale[:1].clone()
        for fold in (0, 1):
            same_bits(launch(nv, case, xc, wc, F32, bias, s, per_col, fold, scratch, ksplit), C.chain(rows, bias, s, F32, fold),
                      f"fp32 per_col={per_col} fold={fold}")
        b16, s16 = bias.bfloat16(), s.bfloat16()
        same_bits(launch(nv, case, xc, wc, BF16, b16, s16, per_col, 0, scratch, ksplit), C.chain(rows, b16, s16, BF16, 0), f"bf16 per_col={per_col}")


def test_plan_split_and_ksplit_one(nv):
    """ksplit = 0 runs the plan's split (four ragged tiles, nk = 8: the plan splits) and ksplit = 1 the unsplit kernel with no
    workspace at all: both equal the host chain."""
    case = "four_tiles"
    ops = C.operands(case)
    rows = ops["exact"].reshape(-1, ops["exact"].shape[-1])
    xc, wc = Margins(ops["x"]), Margins(ops["w"])
    n, h, w, cin, cout, kh, kw = geo_args(case)[:7]
    ks, wb, nt = nv.q8_conv_plan(rows.shape[0], cout, kh * kw * cin)
    assert ks > 1 and wb == 4 * ks * SLAB and nt == 4
    scratch = Scratch(4, ks)
    same_bits(launch(nv, case, xc, wc, F32, None, None, 0, 0, scratch, 0, launches=2), C.chain(rows, None, None, F32, 0), "the plan's split")

    class NoScratch:
        def args(self, ksplit):
            return ksplit, None, 0, None, 0

        def check(self, what):
            pass
    same_bits(launch(nv, case, xc, wc, F32, None, None, 0, 0, NoScratch(), 1), C.chain(rows, None, None, F32, 0), "ksplit = 1")


@pytest.mark.parametrize("case,ksplit", [("one_tile_each", 2), ("mid_pixel_dilation", 7)])
def test_codes_variant_under_a_split(nv, case, ksplit):
    """qt_q8_conv2d_codes_ws against the host's _codes_of_values (the graph's own tail: clamp, CPU quantize, narrowed) on the host
    chain's values, and against the unsplit qt_q8_conv2d_codes; the expected codes are not vacuous."""
    from quantized_training import pt2e_native
    ops = C.operands(case)
    n, h, w, cin, cout, kh, kw = geo_args(case)[:7]
    ho, wo = C.geometry(case)
    rows = ops["exact"].reshape(-1, cout)
    sd = ((256 ** 2 - 1) / 12.0) * (kh * kw * cin) ** 0.5          # standard deviation of a sum of products of uniform codes
    bias, s = ops["bias"].bfloat16(), torch.tensor([1.0 / sd]).bfloat16()
    lo, hi, next_scale = -0.5, 1.5, torch.tensor([2.0 ** -6]).bfloat16()
    v = C.chain(rows, bias, s, BF16, 0)
    y = v.view(n, ho, wo, cout).permute(0, 3, 1, 2)
    want = pt2e_native._codes_of_values(y, lo, hi, next_scale, C.int8_map()).permute(0, 2, 3, 1).reshape(-1, cout)
    c = want.reshape(-1).long()
    assert c.unique().numel() >= 32 and bool(((c > -128) & (c < 127)).float().mean() > 0.25), "the expected codes are vacuous"
    assert int(c.min()) == -32 and int(c.max()) == 96              # both bounds bind: -0.5 * 64, 1.5 * 64
    xc, wc = Margins(ops["x"]), Margins(ops["w"])
    scratch = Scratch(C.tiles_nk(case)[0], ksplit)
    qmap, b, sdev, ns = C.int8_map("cuda"), bias.cuda(), s.cuda(), next_scale.cuda()
    count = rows.numel()
    runs = []
    for split in (True, True, False):
        buf = torch.full((count + 2 * PAD,), 0x5A, dtype=torch.uint8, device="cuda")
        head = (xc.ptr, wc.ptr, buf.data_ptr() + PAD, 0, b.data_ptr(), sdev.data_ptr(), 0, 0, *geo_args(case), 1, lo, hi, ns.data_ptr(),
                qmap.data_ptr())
        if split:
            rc = nv.lib().qt_q8_conv2d_codes_ws(*head, *scratch.args(ksplit), stream())
        else:
            rc = nv.lib().qt_q8_conv2d_codes(*head, stream())
        assert rc == 0
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool((host[:PAD] == 0x5A).all()) and bool((host[PAD + count:] == 0x5A).all()), "a margin of y was written"
        scratch.check(f"{case} codes S={ksplit}")
        runs.append(host[PAD:PAD + count].view(torch.int8).reshape(-1, cout))
    assert torch.equal(runs[0], runs[1]), "two launches differ"
    assert torch.equal(runs[0], runs[2]), "the split codes differ from the unsplit kernel's"
    bad = runs[0] != want
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} codes differ from the host's"


def test_workspace_reuse_reads_no_stale_partial(nv):
    """A large split launch (four tiles, S = 8) followed by a smaller one (one tile, S = 2) in the same workspace: the second equals
    its own reference."""
    big, small = "four_tiles", "one_tile_each"
    scratch = Scratch(4, 8)
    for case, ksplit in ((big, 8), (small, 2), (big, 8)):
        ops = C.operands(case)
        rows = ops["exact"].reshape(-1, ops["exact"].shape[-1])
        xc, wc = Margins(ops["x"]), Margins(ops["w"])
        same_bits(launch(nv, case, xc, wc, F32, None, None, 0, 0, scratch, ksplit), C.chain(rows, None, None, F32, 0), f"{case} in a shared workspace")


def test_ws_entry_points_decline_before_any_launch(nv):
    """A null, short or misaligned workspace or ticket array under a split, ksplit > nk, ksplit < 0 and what the siblings refuse:
    the status, and the output keeps its sentinel."""
    L = nv.lib()
    x = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    w = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    y = torch.full((4096,), float("nan"), dtype=F32, device="cuda")
    ws = torch.zeros(4 * SLAB + 16, dtype=torch.uint8, device="cuda")
    tk = torch.zeros(8, dtype=torch.int32, device="cuda")
    ns, qmap = torch.ones(1, dtype=F32, device="cuda"), C.int8_map("cuda")

    def conv(ksplit=2, wsp=ws.data_ptr(), wsb=4 * SLAB, tkp=tk.data_ptr(), ntk=1, cin=256, xp=x.data_ptr(), codes=False):
        head = (xp, w.data_ptr(), y.data_ptr(), 1, None, None, 0, 0, 1, 4, 4, cin, 16, 1, 1, 1, 1, 0, 0, 1, 1)     # M = 16, nk = cin / 128
        if codes:
            return L.qt_q8_conv2d_codes_ws(*head, 1, 0.0, 6.0, ns.data_ptr(), qmap.data_ptr(), ksplit, wsp, wsb, tkp, ntk, stream())
        return L.qt_q8_conv2d_ws(*head, ksplit, wsp, wsb, tkp, ntk, stream())
    for codes in (False, True):
        assert conv(wsp=None, codes=codes) == nv.QT_ERR_BAD_ARG
        assert conv(tkp=None, codes=codes) == nv.QT_ERR_BAD_ARG
        assert conv(wsb=2 * SLAB - 1, codes=codes) == nv.QT_ERR_BAD_ARG
        assert conv(ntk=0, codes=codes) == nv.QT_ERR_BAD_ARG
        assert conv(wsp=ws.data_ptr() + 8, codes=codes) == nv.QT_ERR_UNALIGNED
        assert conv(tkp=tk.data_ptr() + 2, codes=codes) == nv.QT_ERR_UNALIGNED
        assert conv(ksplit=3, codes=codes) == nv.QT_ERR_BAD_ARG               # nk = 2
        assert conv(ksplit=-1, codes=codes) == nv.QT_ERR_BAD_ARG
        assert conv(ksplit=2, cin=128, codes=codes) == nv.QT_ERR_BAD_ARG      # nk = 1
        assert conv(cin=48, codes=codes) == nv.QT_ERR_BAD_ARG                 # the siblings' refusals
        assert conv(xp=x.data_ptr() + 1, codes=codes) == nv.QT_ERR_UNALIGNED
    torch.cuda.synchronize()
    assert bool(y.isnan().all()) and not bool(tk.any()) and not bool(ws.any())


# ---- the operator and the converted graph ---------------------------------------------------------------------------------------
def op_args(n=2, cin=1024, h=6, w=5, cout=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, cin, h, w, generator=g) * 2).bfloat16().cuda()
    scale = torch.tensor(0.04).bfloat16().cuda()
    wc = torch.randint(-127, 128, (cout, 1, 1, cin), generator=g).to(torch.int8).cuda()
    b = torch.randint(-4000, 4000, (cout,), generator=g).bfloat16().cuda()
    out_scale = torch.tensor([3e-4]).bfloat16().cuda()
    return x, scale, C.int8_map("cuda"), wc, b, out_scale


def test_operator_splits_a_marked_layer(nv, monkeypatch):
    """conv2d_q on a reducing 1 x 1 layer (1024 -> 32, nk = 8, one tile) whose codes buffer carries the mark, the rule bypassed: the
    launch is counted in STATS["conv2d_split_k"] and the result equals the exact chain."""
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    x, scale, qmap, wc, b, out_scale = op_args()
    pt2e_native.mark_split_k(wc)
    before = dict(pt2e_native.STATS)
    y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, wc, b, [1, 1], [0, 0], [1, 1], 1, out_scale, None, "int8")
    ran = {k: pt2e_native.STATS[k] - before.get(k, 0) for k in pt2e_native.STATS}
    assert ran["conv2d_split_k"] == 1 and ran["conv2d_int8"] == 1, ran
    xq = torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap).cpu()
    exact = C.conv_exact(xq, wc.cpu().permute(0, 3, 1, 2), [1, 1], [0, 0], [1, 1])
    same_bits(y.permute(0, 2, 3, 1).reshape(-1, 32).cpu(), C.chain(exact, b.cpu(), out_scale.cpu(), BF16, 0).reshape(-1, 32), "marked layer")


def test_operator_leaves_an_unmarked_layer_alone(nv):
    """The same layer without the mark, the committed rules on: the three nodes run, nothing is counted, the reason is the parent's."""
    from quantized_training import pt2e_native
    x, scale, qmap, wc, b, out_scale = op_args()
    before, why = dict(pt2e_native.STATS), "route rule: profiles/conv2d_q.txt"
    reasons = pt2e_native.CONV_Q_REASONS.get(why, 0)
    y = torch.ops.quantized_ops.conv2d_q(x, scale, qmap, wc, b, [1, 1], [0, 0], [1, 1], 1, out_scale, None, "int8")
    assert pt2e_native.STATS == before and pt2e_native.CONV_Q_REASONS.get(why, 0) == reasons + 1
    xq = torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap)
    v = torch.nn.functional.conv2d(xq, wc.permute(0, 3, 1, 2).bfloat16().contiguous(), b)
    want = torch.ops.quantized_ops.dequantize(v, out_scale, None, None, None, None)
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


def test_converted_cnn_with_split_k(nv, monkeypatch):
    """ProjectNet converted with split_k=True, the rule bypassed: the projecting layer's launch is a split one; layer by layer every
    conv2d_q equals the exact chain on its own input; a torch.cuda.graph capture replayed three times equals the eager call."""
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    gm, x = C.convert_project_net(monkeypatch, "cuda", split_k=True)
    assert C.call_targets(gm).count("quantized_ops.conv2d_q.default") == 2
    before = dict(pt2e_native.STATS)
    with torch.no_grad():
        eager = gm(x).clone()
    ran = {k: pt2e_native.STATS[k] - before.get(k, 0) for k in pt2e_native.STATS}
    assert ran["conv2d_int8"] == 2 and ran["conv2d_split_k"] == 1, ran          # expand: nk = 1, never split; project: nk = 8
    checked = []

    class PerLayer(torch.fx.Interpreter):
        def call_function(self, target, args, kwargs):
            out = super().call_function(target, args, kwargs)
            if target == torch.ops.quantized_ops.conv2d_q.default:
                inp, scale, qmap, wc, b, stride, padding, dilation, groups, out_scale, out_map, _ = args
                xq = torch.ops.quantized_ops.quantize(inp, scale, None, None, None, qmap).cpu()
                exact = C.conv_exact(xq, wc.cpu().permute(0, 3, 1, 2), stride, padding, dilation)
                want = C.chain(exact, b.cpu(), out_scale.cpu().reshape(-1), inp.dtype, 0)
                same_bits(out.permute(0, 2, 3, 1).reshape(-1, wc.shape[0]).cpu(), want.reshape(-1, wc.shape[0]), f"layer {tuple(wc.shape)}")
                checked.append(wc.shape[0])
            return out
    with torch.no_grad():
        PerLayer(gm).run(x)
    assert checked == [1024, 32]

    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        gm(static_x)                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    before = pt2e_native.STATS["conv2d_split_k"]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = gm(static_x)
    assert pt2e_native.STATS["conv2d_split_k"] - before == 1          # the capture took the split launch
    static_x.copy_(x)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))


def test_converted_cnn_chains_into_the_projecting_layer(nv, monkeypatch):
    """split_k=True with chain_convs=True, the rule bypassed: the edge into the projecting layer is a pair of conv2d_qc nodes and the
    output equals the un-chained graph's."""
    from quantized_training import pt2e_native
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    plain, x = C.convert_project_net(monkeypatch, "cuda", split_k=True)
    chained, _ = C.convert_project_net(monkeypatch, "cuda", split_k=True, chain_convs=True)
    t = C.call_targets(chained)
    assert t.count("quantized_ops.conv2d_qc.default") == 2 and t.count("quantized_ops.conv2d_q.default") == 0, t
    before = dict(pt2e_native.STATS)
    with torch.no_grad():
        y0, y1 = plain(x), chained(x)
    ran = {k: pt2e_native.STATS[k] - before.get(k, 0) for k in pt2e_native.STATS}
    assert ran["conv2d_codes_out"] == 1 and ran["conv2d_codes_in"] == 1 and ran["conv2d_split_k"] == 2, ran          # the projecting layer of either graph
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
