"""qt_linear_gwa_tall_bf16 (csrc/qt_gwa_tall.hip) on the device: both row tiles, every split of K, the operator's "tall" route.
The tiers and the problem builders are test_gpu_gwa_gemm.py's; its derived bound u_out |y64| + (K + 12) u S counts the partial sums
of at most 8 ranges of K, and the tall kernel splits K 8 ways at the most, so the bound holds verbatim."""
import pytest
import torch
import torch.nn.functional as F

from kernel_launch import nv, stream  # noqa: F401
from test_gpu_gwa_gemm import (GuardedY, _leave_no_routes, bits, bound_of, dequantize_op, exact_problem, native, pack,  # noqa: F401
                               real_problem)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
TILES, SPLITS = [128, 256], [1, 2, 4, 8]


def scratch(M, N, bm, split):
    """A NaN-filled workspace and zeroed tickets of exactly the size the header's formulas give."""
    tiles = -(-M // bm) * -(-N // 128)
    ws = torch.full((tiles * split * bm * 128,), float("nan"), dtype=torch.float32, device="cuda") if split > 1 else None
    return ws, torch.zeros(tiles, dtype=torch.int32, device="cuda") if split > 1 else None


def launch(nv, x, packed, s, z, bias, y, K, bs, nbits, qmin, bm, split, ws, tickets):
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    n = lambda t: t.numel() if t is not None else 0  # noqa: E731
    return nv.lib().qt_linear_gwa_tall_bf16(ptr(x), ptr(packed), ptr(s), ptr(z), ptr(bias), ptr(y), y.shape[0], y.shape[1], K, bs, nbits, float(qmin),
                                            bm, split, ptr(ws), n(ws) * 4, ptr(tickets), n(tickets), stream())


def run(nv, x, packed, s, z, bias, bs, qmin, nbits, bm, split, N):
    """x inside a larger buffer whose margins are NaN, y between guards, the workspace NaN, the tickets zero afterwards."""
    M, K = x.shape
    big = torch.full((M * K + 256,), float("nan"), dtype=BF16, device="cuda")
    xin = big[128:128 + M * K].view(M, K)                                   # what lies past the last row's K is NaN
    xin.copy_(x)
    gy = GuardedY(M, N)
    ws, tickets = scratch(M, N, bm, split)
    assert launch(nv, xin, packed, s, z, bias, gy.y, K, bs, nbits, qmin, bm, split, ws, tickets) == 0
    torch.cuda.synchronize()
    assert gy.intact(), "guard region of y overwritten"
    assert not bool(torch.isnan(gy.y).any()), "an element of y was not written, or a value outside x was multiplied"
    assert tickets is None or not bool(tickets.any()), "tickets are not zero after the launch"
    return gy.y


IDENTITY = [("uint4", 32), ("uint4", 128), ("int4", 32), ("uint8", 32), ("uint4-e5m3", 32)]


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("bm", TILES)
@pytest.mark.parametrize("K", [96, 256])               # 96: a partial k tile and a partial 4-bit super step
@pytest.mark.parametrize("kind,bs", IDENTITY, ids=[f"{k}-bs{b}" for k, b in IDENTITY])
def test_identity_activation_reads_back_the_dequantize_operators_weight(nv, kind, bs, K, bm, split):
    N = 40
    bs = bs if K % bs == 0 else 32
    codes, s, z, qmin, qmax, nbits = real_problem(kind, N, K, bs, seed=K + bs)
    wd = dequantize_op(codes, s, z, bs)
    y = run(nv, torch.eye(K, dtype=BF16, device="cuda"), pack(nv, codes, qmin, qmax, nbits), s, z, None, bs, qmin, nbits, bm, split, N)
    diff = bits(y) != bits(wd.t())
    assert not bool(diff.any()), f"{int(diff.sum())} of {diff.numel()} elements differ from dequantize"


# ragged M and a half-valid column group in a second tile | 34 super steps (the ring wraps, an uneven split, a row tile of one row) |
# 8 bits | a block spanning four super steps | four blocks per super step, K % 64 = 32 | M far below a tile
EXACT = [(129, 136, 384, 128, "uint4"), (257, 24, 4352, 128, "uint4"), (300, 136, 384, 128, "uint8"), (130, 264, 1536, 512, "uint4"),
         (128, 128, 160, 32, "uint4"), (17, 16, 256, 256, "uint2")]
_exact = {}


def exact_case(M, N, K, bs, kind):
    """The problem, its packed weight and the two expected results, built once per shape and left unchanged."""
    key = (M, N, K, bs, kind)
    if key not in _exact:
        x, codes, s, z, bias, qmin, qmax, nbits = exact_problem(M, N, K, bs, kind, seed=M + N + K + bs)
        wd = dequantize_op(codes, s, z, bs).double()
        S = x.double().abs() @ wd.abs().t() + bias.double().abs()
        assert float(S.max()) < 2 ** 24 * (0.25 if nbits == 4 else 1.0), "the problem is not exact in fp32"
        y64 = x.double() @ wd.t()
        _exact[key] = (x, native().gwa_pack(codes, qmin, qmax, nbits), s, z, bias, qmin, nbits, (y64 + bias.double()).to(BF16), y64.to(BF16))
    return _exact[key]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("bm", TILES)
@pytest.mark.parametrize("M,N,K,bs,kind", EXACT, ids=[f"{m}x{n}x{k}-bs{b}-{d}" for m, n, k, b, d in EXACT])
def test_exact_tier_equals_the_fp64_product_rounded_once(nv, M, N, K, bs, kind, bm, split):
    x, packed, s, z, bias, qmin, nbits, with_bias, without = exact_case(M, N, K, bs, kind)
    for b, exp in ((bias, with_bias), (None, without)):
        y = run(nv, x, packed, s, z, b, bs, qmin, nbits, bm, split, N)
        diff = bits(y) != bits(exp)
        assert not bool(diff.any()), f"{int(diff.sum())} of {diff.numel()} elements differ, first at {diff.nonzero()[0].tolist()}"


TOL = [(300, 136, 1536, 128, "uint4"), (129, 72, 768, 64, "uint8")]


@pytest.mark.parametrize("M,N,K,bs,kind", TOL, ids=[f"{m}x{n}x{k}-bs{b}-{d}" for m, n, k, b, d in TOL])
def test_tolerance_tier_against_fp64_and_route_a(nv, M, N, K, bs, kind):
    codes, s, z, qmin, qmax, nbits = real_problem(kind, N, K, bs, seed=M + K, all_codes=False)
    g = torch.Generator().manual_seed(M * N)
    x, bias = torch.randn(M, K, generator=g).to(BF16).cuda(), torch.randn(N, generator=g).to(BF16).cuda()
    wd = dequantize_op(codes, s, z, bs)
    y64 = x.double() @ wd.double().t() + bias.double()
    bound = bound_of(y64, x.double().abs() @ wd.double().abs().t() + bias.double().abs(), K)
    aerr = (F.linear(x, wd, bias).double() - y64).abs()                          # route (a)
    packed = pack(nv, codes, qmin, qmax, nbits)
    for bm in TILES:
        for split in SPLITS:
            err = (run(nv, x, packed, s, z, bias, bs, qmin, nbits, bm, split, N).double() - y64).abs()
            print(f"\n[gwa tall {M}x{N}x{K} {kind} tile {bm} split {split}] largest error / bound {float((err / bound).max()):.3f}, route (a) {float((aerr / bound).max()):.3f}")
            assert bool((err <= bound).all()), f"tile {bm} split {split}: worst ratio {float((err / bound).max())}"
            assert bool((err <= aerr + bound).all()), f"tile {bm} split {split}: worse than route (a) by more than the bound"


def test_two_runs_and_graph_replays_of_a_split_launch_are_bit_equal(nv):
    M, N, K, bs, split = 130, 264, 2048, 128, 8
    codes, s, z, qmin, qmax, nbits = real_problem("uint4", N, K, bs, seed=3, all_codes=False)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(1)).to(BF16).cuda()
    packed = pack(nv, codes, qmin, qmax, nbits)
    a = run(nv, x, packed, s, z, None, bs, qmin, nbits, 128, split, N)
    b = run(nv, x, packed, s, z, None, bs, qmin, nbits, 128, split, N)
    assert torch.equal(bits(a), bits(b))
    out = torch.zeros(M, N, dtype=BF16, device="cuda")
    ws, tickets = scratch(M, N, 128, split)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert launch(nv, x, packed, s, z, None, out, K, bs, nbits, qmin, 128, split, ws, tickets) == 0
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(a)) and not bool(tickets.any())


REFUSALS = [(dict(bm=64), "BAD"), (dict(bm=512), "BAD"), (dict(split=3), "BAD"), (dict(split=16), "BAD"), (dict(ws="none"), "BAD"),
            (dict(tickets="none"), "BAD"), (dict(ws="short"), "BAD"), (dict(tickets="short"), "BAD"), (dict(ws="off"), "UNAL")]


@pytest.mark.parametrize("kw,code", REFUSALS, ids=[f"{k}-{v}" for r in REFUSALS for k, v in r[0].items()])
def test_every_new_refusal_leaves_y_alone(nv, kw, code):
    M, N, K, bs, split = 130, 136, 256, 128, 2
    x, packed, s, z, bias, qmin, nbits, *_ = exact_case(M, N, K, bs, "uint4")
    gy = GuardedY(M, N)
    ws, tickets = scratch(M, N, 128, split)
    variants = {"ws": {"none": None, "short": ws[:-1], "off": torch.cat([ws, ws[:4]])[1:1 + ws.numel()]}, "tickets": {"none": None, "short": tickets[:-1]}}
    a = dict(bm=128, split=split, ws=ws, tickets=tickets)
    a.update({k: variants[k][v] if k in variants else v for k, v in kw.items()})
    rc = launch(nv, x, packed, s, z, bias, gy.y, K, bs, nbits, qmin, a["bm"], a["split"], a["ws"], a["tickets"])
    assert rc == (nv.QT_ERR_BAD_ARG if code == "BAD" else nv.QT_ERR_UNALIGNED)
    torch.cuda.synchronize()
    assert gy.untouched()


def test_operator_tall_route_counts_reports_and_equals_the_direct_launch(nv):
    from quantized_training import fused as fz
    pn = native()
    M, N, K, bs = 130, 136, 512, 128
    codes, s, z, qmin, qmax, nbits = real_problem("uint4", N, K, bs, seed=4, all_codes=False)
    x = torch.randn(2, M // 2, K, generator=torch.Generator().manual_seed(8)).to(BF16).cuda()
    bias = torch.randn(N, generator=torch.Generator().manual_seed(9)).to(BF16).cuda()
    packed = pack(nv, codes, qmin, qmax, nbits)
    pn.GWA_STATS.reset()
    pn.GWA_ROUTES.clear()
    for bm, split in ((0, 0), (256, 2)):
        got = pn.linear_gwa_route(x, packed, s, z, bias, bs, qmin, nbits, K, route="tall", tile_m=bm, split=split)
        plan = nv.gwa_tall_plan(M, N, K, nbits, bm)
        direct = run(nv, x.view(M, K), packed, s, z, bias, bs, qmin, nbits, plan[0], split or plan[1], N)
        assert got.shape == (2, M // 2, N) and torch.equal(bits(got.view(M, N)), bits(direct))
    assert (pn.GWA_STATS.tall, pn.GWA_STATS.fused, pn.GWA_STATS.dequant) == (2, 0, 0)
    assert fz.routes_report().get(f"gwa:{M}x{N}x{K}") == "fused_gwa_tall_gemm"
    # a variant the kernel declines falls to the dequantize kernel + the library GEMM
    got = pn.linear_gwa_route(x, packed, s, z, bias, bs, qmin, nbits, K, route="tall", tile_m=64)
    assert pn.GWA_STATS.dequant == 1 and pn.GWA_STATS.reasons == {"qt_linear_gwa_tall_bf16 declined": 1}
    assert torch.equal(bits(got), bits(F.linear(x, dequantize_op(codes, s, z, bs), bias)))
    # the committed rules: M = 33 over a small weight is in neither, it stays with route (b)
    pn.GWA_STATS.reset()
    torch.ops.quantized_ops.linear_gwa(x.view(M, K)[:33], packed, s, z, bias, bs, qmin, nbits, K)
    assert not pn._gwa_tall_route_takes(33, N, K, nbits)
    assert pn.GWA_STATS.dequant == 1 and pn.GWA_STATS.reasons == {"route rule": 1}
