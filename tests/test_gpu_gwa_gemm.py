"""Packed group-wise affine weights on the device (csrc/qt_gwa_gemm.hip): qt_gwa_pack, qt_gwa_dequantize_bf16, qt_linear_gwa_bf16 in
every tile height it ships, the linear_gwa operator's routes, and the graph pass on a device model.

    y[m][n] = rd( bias[n] + sum_k x[m][k] Wd[n][k] ),     Wd[n][k] = rd(rd(q[n][k] - z[n][k / bs]) * s[n][k / bs]),   rd = round to bf16

Wd must be, bit for bit, what quantized_ops.dequantize makes of the bf16 codes: the identity test reads it back through the GEMM
(x = I adds one exact product to exact zeros), for every code value in every block and the non-integer zero points of the real
fake-quantizer.

Exact tier: small-integer x, integer zero points, power-of-two scales and a bias on the same grid make every product and every
partial sum of any summation order an fp32 number (the test asserts sum_k |x Wd| + |bias| < 2^24 quanta), so the result is the
fp64 product rounded once to bf16, bit for bit.

Tolerance tier (derived, not measured): a product of two bf16 numbers is exact in fp32 (16 significant bits); the kernel adds the
K products of an output, the partial sums of at most 8 K ranges and the bias in fp32 -- fewer than K + 9 additions whatever the
order inside the matrix instruction, each rounding (u = 2^-24) a partial sum bounded by S = sum_k |x Wd| + |bias| -- and rounds
once to bf16 (u_out = 2^-8):
    |y - y64| <= u_out |y64| + (K + 12) u S          (+ 3: second-order terms, among them u_out acting on the accumulation error)
Route (a), dequantize + aten.linear on the same bf16 operands, obeys the same bound; the fused result's error must not exceed
route (a)'s by more than that bound either.
"""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from kernel_launch import nv, stream  # noqa: F401
from test_gwa_gemm_cpu import DQ, GWA, LIN, prepared, rows, targets

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
U = 2.0 ** -24
TILES = [0, 16, 32, 64]
SPECS = {"uint4": "uint4,qs=group_wise_affine,bs={bs},ax=-1", "int4": "int4,qs=group_wise_affine,bs={bs},ax=-1",
         "uint2": "uint2,qs=group_wise_affine,bs={bs},ax=-1", "uint8": "uint8,qs=group_wise_affine,bs={bs},ax=-1",
         "uint4-e5m3": "uint4,qs=group_wise_affine,bs={bs},ax=-1,scale=fp8_e5m3"}


@pytest.fixture(autouse=True)
def _leave_no_routes():
    """routes_report() of later tests lists what THEY ran: the process-wide table of linear_gwa routes is put back as this test found it."""
    from quantized_training import pt2e_native
    before = dict(pt2e_native.GWA_ROUTES)
    yield
    pt2e_native.GWA_ROUTES.clear()
    pt2e_native.GWA_ROUTES.update(before)


def bits(t):
    return t.detach().contiguous().view(torch.int16)


def native():
    from quantized_training import pt2e_native
    return pt2e_native


def at_end(t):
    """A copy of t whose last byte is the last byte of its allocation's requested size, 16-byte aligned."""
    n = t.numel() * t.element_size()
    pad = 256
    raw = torch.empty(pad + n, dtype=torch.uint8, device="cuda")
    v = raw[pad:].view(t.dtype).view(t.shape)
    v.copy_(t)
    return v


class GuardedY:
    """y between two guard regions of 0xFF bytes (bf16 NaN patterns)."""
    G = 256

    def __init__(self, M, N):
        self.n = M * N * 2
        self.raw = torch.full((self.n + 2 * self.G,), 0xFF, dtype=torch.uint8, device="cuda")
        self.y = self.raw[self.G:self.G + self.n].view(BF16).view(M, N)

    def intact(self):
        return bool((self.raw[:self.G] == 0xFF).all()) and bool((self.raw[self.G + self.n:] == 0xFF).all())

    def untouched(self):
        return bool((self.raw == 0xFF).all())


def real_problem(kind, N, K, bs, seed=0, all_codes=True):
    """Codes, scales and zero points of a random weight from the actual fake-quantizer (what _lower_group_wise_affine stores), with
    -- all_codes -- the codes replaced so that every block holds every code value (as often as it fits), shuffled."""
    import quantized_training as qt
    from dataclasses import asdict
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * (1 + torch.rand(N, 1, generator=g) * 3) + 0.3).to(BF16).cuda()
    fq = qt.FusedAmaxObsFakeQuantize(**asdict(qt.QuantizationSpec.from_str(SPECS[kind].format(bs=bs))), device="cuda")
    fq(w)
    s, z = fq.calculate_qparams()
    s, z = s.to(BF16).contiguous(), z.to(BF16).contiguous()
    codes = torch.ops.quantized_ops.quantize(w, s, z, [-1], bs, fq.qmap)
    qmin, qmax, nbits = native().gwa_dtype_range(kind.split("-")[0])
    if all_codes:
        span = qmax - qmin + 1
        blk = torch.arange(N * (K // bs)).view(N, K // bs, 1)                  # (256 codes in blocks of 32: eight blocks hold them all)
        base = ((torch.arange(bs) + blk * bs) % span + qmin).to(torch.float32)
        perm = torch.rand(N, K // bs, bs, generator=g).argsort(-1)
        codes = torch.gather(base, -1, perm).view(N, K).to(BF16).cuda()
    assert float(z.float().frac().abs().max()) > 0 or kind == "uint4-e5m3", "zero points are expected not to be integers"
    return codes, s, z, qmin, qmax, nbits


def pack(nv, codes, qmin, qmax, nbits):
    p = native().gwa_pack(codes, qmin, qmax, nbits)
    assert p is not None
    return p


def run(nv, x, packed, s, z, bias, bs, qmin, nbits, tile, N, out=None):
    M, K = x.shape
    gy = GuardedY(M, N) if out is None else None
    y = gy.y if out is None else out
    rc = nv.lib().qt_linear_gwa_bf16(x.data_ptr(), packed.data_ptr(), s.data_ptr(), z.data_ptr(), bias.data_ptr() if bias is not None else None,
                                     y.data_ptr(), M, N, K, bs, nbits, float(qmin), tile, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    if gy is not None:
        assert gy.intact(), "guard region of y overwritten"
        assert not bool(torch.isnan(y).any()), "an element of y was not written"
    return y


def dequantize_op(codes, s, z, bs):
    return torch.ops.quantized_ops.dequantize(codes, s, z, (-1,), bs)


# ---- 1. the dequantized operand, bit for bit --------------------------------------------------------------------------------------------
IDENTITY = [("uint4", 64, 32), ("uint4", 128, 128), ("uint4", 256, 64), ("uint4", 256, 256), ("int4", 128, 32), ("uint2", 64, 64),
            ("uint8", 256, 256), ("uint8", 128, 32), ("uint4-e5m3", 128, 64)]


@pytest.mark.parametrize("kind,K,bs", IDENTITY, ids=[f"{k}-K{K}-bs{b}" for k, K, b in IDENTITY])
def test_identity_activation_reads_back_the_dequantize_operators_weight(nv, kind, K, bs):
    N = 40
    codes, s, z, qmin, qmax, nbits = real_problem(kind, N, K, bs, seed=K + bs)
    if nbits == 8 and bs < 256:
        assert codes.unique().numel() == 256                                   # all 256 codes, over the tensor
    else:
        assert all(b.unique().numel() == qmax - qmin + 1 for b in codes.view(N, K // bs, bs)[::7, 0])
    wd = dequantize_op(codes, s, z, bs)
    packed = pack(nv, codes, qmin, qmax, nbits)
    assert torch.equal(packed.cpu(), native().gwa_pack_torch(codes.cpu(), qmin, qmax, nbits)), "device packer vs the torch-op layout"
    # qt_gwa_dequantize_bf16
    w2 = native().gwa_dequantize(packed, s, z, bs, qmin, nbits, K)
    assert torch.equal(bits(w2), bits(wd)), f"qt_gwa_dequantize_bf16: {int((bits(w2) != bits(wd)).sum())} elements differ"
    x = torch.eye(K, dtype=BF16, device="cuda")
    for tile in TILES:
        y = run(nv, x, packed, s, z, None, bs, qmin, nbits, tile, N)
        diff = bits(y) != bits(wd.t())
        assert not bool(diff.any()), f"tile {tile}: {int(diff.sum())} of {diff.numel()} elements differ from dequantize"


# ---- 2. exact tier -------------------------------------------------------------------------------------------------------------------------
def exact_problem(M, N, K, bs, kind, seed):
    g = torch.Generator().manual_seed(seed)
    qmin, qmax, nbits = native().gwa_dtype_range(kind)
    wide = nbits == 8
    x = torch.randint(-2 if wide else -4, (2 if wide else 4) + 1, (M, K), generator=g).to(BF16)
    codes = torch.randint(qmin, qmax + 1, (N, K), generator=g).to(BF16)
    z = torch.randint(qmin, qmax + 1, (N, K // bs), generator=g).to(BF16)
    exps = torch.randint(0, 2, (N, K // bs), generator=g) if wide else torch.randint(-2, 2, (N, K // bs), generator=g)
    s = (2.0 ** exps.float()).to(BF16)
    bias = (torch.randint(-64, 65, (N,), generator=g).float() * 0.25).to(BF16)
    return [t.cuda() for t in (x, codes, s, z, bias)] + [qmin, qmax, nbits]


# M, N, K, bs, kind.  K = 4352 is 34 (4 bits) / 68 (8 bits) super steps: more than the 8 x 4 ring slots of a workgroup's eight waves
EXACT = [(1, 8, 32, 32, "uint4"), (15, 16, 96, 32, "uint4"), (16, 24, 64, 64, "int4"), (17, 136, 192, 64, "uint4"),
         (129, 24, 128, 128, "uint4"), (300, 136, 384, 128, "uint8"), (17, 16, 256, 256, "uint2"), (129, 8, 768, 256, "uint4"),
         (15, 24, 512, 512, "uint8"), (300, 16, 1536, 512, "uint4"), (17, 24, 4352, 128, "uint4"), (129, 16, 4352, 64, "uint8")]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("M,N,K,bs,kind", EXACT, ids=[f"{m}x{n}x{k}-bs{b}-{d}" for m, n, k, b, d in EXACT])
def test_exact_tier_equals_the_fp64_product_rounded_once(nv, M, N, K, bs, kind, tile):
    x, codes, s, z, bias, qmin, qmax, nbits = exact_problem(M, N, K, bs, kind, seed=M + N + K + bs)
    wd = dequantize_op(codes, s, z, bs)
    quantum = 0.25 if nbits == 4 else 1.0
    S = x.double().abs() @ wd.double().abs().t() + bias.double().abs()
    assert float(S.max()) < 2 ** 24 * quantum, "the problem is not exact in fp32"
    y64 = x.double() @ wd.double().t() + bias.double()
    packed = pack(nv, codes, qmin, qmax, nbits)
    y = run(nv, x, packed, s, z, bias, bs, qmin, nbits, tile, N)
    exp = y64.to(BF16)
    diff = bits(y) != bits(exp)
    assert not bool(diff.any()), f"{int(diff.sum())} of {diff.numel()} elements differ, first at {diff.nonzero()[0].tolist()}"
    if tile == 0:                                                               # without a bias
        y0 = run(nv, x, packed, s, z, None, bs, qmin, nbits, tile, N)
        assert torch.equal(bits(y0), bits((x.double() @ wd.double().t()).to(BF16)))


# ---- 3. tolerance tier --------------------------------------------------------------------------------------------------------------------
def bound_of(y64, S, K):
    return 2.0 ** -8 * y64.abs() + (K + 12) * U * S + 1e-300


TOL = [(1, 136, 512, 128, "uint4"), (16, 136, 384, 128, "uint4-e5m3"), (48, 72, 256, 32, "int4"), (130, 136, 512, 64, "uint8"),
       (300, 24, 1024, 256, "uint4")]


@pytest.mark.parametrize("M,N,K,bs,kind", TOL, ids=[f"{m}x{n}x{k}-bs{b}-{d}" for m, n, k, b, d in TOL])
def test_tolerance_tier_against_fp64_and_route_a(nv, M, N, K, bs, kind):
    """The module docstring's bound, for the kernel's own choice of tile and for every forced one."""
    codes, s, z, qmin, qmax, nbits = real_problem(kind, N, K, bs, seed=M + K, all_codes=False)
    g = torch.Generator().manual_seed(M * N)
    x = torch.randn(M, K, generator=g).to(BF16).cuda()
    bias = torch.randn(N, generator=g).to(BF16).cuda()
    wd = dequantize_op(codes, s, z, bs)
    y64 = x.double() @ wd.double().t() + bias.double()
    S = x.double().abs() @ wd.double().abs().t() + bias.double().abs()
    bound = bound_of(y64, S, K)
    aerr = (F.linear(x, wd, bias).double() - y64).abs()                          # route (a)
    packed = pack(nv, codes, qmin, qmax, nbits)
    for tile in TILES:
        y = run(nv, x, packed, s, z, bias, bs, qmin, nbits, tile, N)
        err = (y.double() - y64).abs()
        print(f"\n[gwa {M}x{N}x{K} {kind} tile {tile}] largest error / bound {float((err / bound).max()):.3f}, route (a) {float((aerr / bound).max()):.3f}")
        assert bool((err <= bound).all()), f"tile {tile}: {int((err > bound).sum())} elements outside the bound, worst ratio {float((err / bound).max())}"
        assert bool((err <= aerr + bound).all()), f"tile {tile}: worse than route (a) by more than the bound"


# ---- 4. guards, buffers that end at their last byte, determinism, capture ---------------------------------------------------------------
def test_operands_that_end_at_their_last_byte_and_ragged_edges(nv):
    M, N, K, bs = 19, 24, 96, 32                              # ragged M, a half-filled last column group, a ragged last super step
    x, codes, s, z, bias, qmin, qmax, nbits = exact_problem(M, N, K, bs, "uint4", seed=5)
    exp = (x.double() @ dequantize_op(codes, s, z, bs).double().t() + bias.double()).to(BF16)
    packed = pack(nv, at_end(codes), qmin, qmax, nbits)
    assert packed.numel() == 2 * 1 * 1024
    xe, pe, se, ze, be = at_end(x), at_end(packed), at_end(s), at_end(z), at_end(bias)
    for tile in TILES:
        y = run(nv, xe, pe, se, ze, be, bs, qmin, nbits, tile, N)
        assert torch.equal(bits(y), bits(exp)), tile
    w = GuardedY(N, K)
    assert nv.lib().qt_gwa_dequantize_bf16(pe.data_ptr(), se.data_ptr(), ze.data_ptr(), w.y.data_ptr(), N, K, bs, nbits, float(qmin), stream()) == 0
    torch.cuda.synchronize()
    assert w.intact() and torch.equal(bits(w.y), bits(dequantize_op(codes, s, z, bs)))


def test_two_runs_and_a_graph_replay_are_bit_equal(nv):
    for M, K in ((16, 4352), (130, 512)):                     # one row tile with full rings; three row tiles of 64
        N, bs = 72, 128
        codes, s, z, qmin, qmax, nbits = real_problem("uint4", N, K, bs, seed=3, all_codes=False)
        x = torch.randn(M, K, generator=torch.Generator().manual_seed(1)).to(BF16).cuda()
        packed = pack(nv, codes, qmin, qmax, nbits)
        a = run(nv, x, packed, s, z, None, bs, qmin, nbits, 0, N)
        b = run(nv, x, packed, s, z, None, bs, qmin, nbits, 0, N)
        assert torch.equal(bits(a), bits(b))
        out = torch.zeros(M, N, dtype=BF16, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = nv.lib().qt_linear_gwa_bf16(x.data_ptr(), packed.data_ptr(), s.data_ptr(), z.data_ptr(), None, out.data_ptr(), M, N, K, bs,
                                             nbits, float(qmin), 0, stream())
        assert rc == 0
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(a))


# ---- 5. the packer's flag ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0.5, 16.0, -1.0, float("nan")], ids=["fraction", "above", "below", "nan"])
def test_packer_flags_a_planted_code(nv, bad):
    codes = torch.randint(0, 16, (24, 160), generator=torch.Generator().manual_seed(2)).to(BF16).cuda()
    assert native().gwa_pack(codes, 0, 15, 4) is not None
    codes[23, 159] = bad
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    packed = torch.empty(nv.lib().qt_gwa_packed_bytes(24, 160, 4), dtype=torch.uint8, device="cuda")
    assert nv.lib().qt_gwa_pack(codes.data_ptr(), packed.data_ptr(), 24, 160, 4, 0.0, 15.0, flag.data_ptr(), stream()) == 0
    assert int(flag.item()) == 1
    assert native().gwa_pack(codes, 0, 15, 4) is None


class TwoLinears(nn.Module):
    def __init__(self, k=256, h=512, n=136):
        super().__init__()
        self.fc1 = nn.Linear(k, h)
        self.fc2 = nn.Linear(h, n, bias=False)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x)))


def converted(native_flag, plant=None, spec="uint4,qs=group_wise_affine,bs=128,ax=-1"):
    from quantized_training import quantize_pt2e as qp
    torch.manual_seed(0)
    m = TwoLinears().eval().to(BF16).cuda()
    x = torch.randn(4, 256).to(BF16).cuda()
    gm = prepared(spec, m, x)
    if plant is None:
        return qp.convert_pt2e(gm, native=native_flag), x
    plain = qp.convert_pt2e(gm, native=False)
    plant(plain)
    return plain, x


def test_pass_keeps_the_unfused_graph_for_a_weight_with_a_bad_code(nv):
    def plant(gm):
        q = [n for n in gm.graph.nodes if str(n.target) == DQ][0].args[0]
        gm.get_buffer(q.target)[5, 9] = 0.5
    gm, x = converted(False, plant)
    before = rows(gm)
    assert native().fuse_gwa_linears(gm) == 1
    after = [r for r in rows(gm)]
    first_dq = [r for r in before if r[1] == DQ][0]
    assert first_dq in after and targets(gm).count(DQ) == 1 and targets(gm).count(LIN) == 1 and targets(gm).count(GWA) == 1


# ---- 6. declines ---------------------------------------------------------------------------------------------------------------------------
def test_every_decline_of_the_entry_points_leaves_the_outputs_alone(nv):
    L, BAD, UNAL = nv.lib(), nv.QT_ERR_BAD_ARG, nv.QT_ERR_UNALIGNED
    M, N, K, bs = 4, 16, 128, 128
    x, codes, s, z, bias, qmin, qmax, nbits = exact_problem(M, N, K, bs, "uint4", seed=9)
    packed = pack(nv, codes, qmin, qmax, nbits)
    gy = GuardedY(M, N)
    p = dict(x=x.data_ptr(), packed=packed.data_ptr(), s=s.data_ptr(), z=z.data_ptr(), bias=bias.data_ptr(), y=gy.y.data_ptr(), M=M, N=N, K=K,
             bs=bs, bits=4, qmin=0.0, tile=0)

    def gemm(**kw):
        a = dict(p, **kw)
        return L.qt_linear_gwa_bf16(a["x"], a["packed"], a["s"], a["z"], a["bias"], a["y"], a["M"], a["N"], a["K"], a["bs"], a["bits"], a["qmin"],
                                    a["tile"], stream())
    for name in ("x", "packed", "s", "z", "y"):
        assert gemm(**{name: None}) == BAD, name
    for kw in (dict(bits=2), dict(bits=16), dict(bs=16), dict(bs=96), dict(bs=1024), dict(N=0), dict(K=0), dict(M=-1), dict(tile=8), dict(tile=128)):
        assert gemm(**kw) == BAD, kw
    for kw in (dict(K=192), dict(K=144), dict(N=12), dict(N=20), dict(x=p["x"] + 2), dict(packed=p["packed"] + 8), dict(y=p["y"] + 8),
               dict(s=p["s"] + 1), dict(z=p["z"] + 1), dict(bias=p["bias"] + 4), dict(K=64, bs=128)):
        assert gemm(**kw) == UNAL, kw
    assert gemm(M=0) == 0
    torch.cuda.synchronize()
    assert gy.untouched()
    # qt_gwa_dequantize_bf16
    gw = GuardedY(N, K)

    def deq(packed=p["packed"], s=p["s"], z=p["z"], y=gw.y.data_ptr(), N=N, K=K, bs=bs, bits=4):
        return L.qt_gwa_dequantize_bf16(packed, s, z, y, N, K, bs, bits, 0.0, stream())
    assert [deq(packed=None), deq(s=None), deq(z=None), deq(y=None), deq(bits=3), deq(bs=48), deq(N=0)] == [BAD] * 7
    assert [deq(K=160), deq(N=12), deq(packed=p["packed"] + 4), deq(y=gw.y.data_ptr() + 2), deq(s=p["s"] + 1), deq(K=64)] == [UNAL] * 6
    torch.cuda.synchronize()
    assert gw.untouched()
    # qt_gwa_pack
    out = torch.full((1024 + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def pk(codes=codes.data_ptr(), out=out.data_ptr(), N=N, K=K, bits=4, lo=0.0, hi=15.0):
        return L.qt_gwa_pack(codes, out, N, K, bits, lo, hi, flag.data_ptr(), stream())
    assert [pk(codes=None), pk(out=None), pk(bits=5), pk(hi=16.0), pk(lo=0.5), pk(lo=3.0, hi=2.0), pk(bits=8, hi=256.0), pk(N=0)] == [BAD] * 8
    assert [pk(K=48), pk(N=12), pk(codes=codes.data_ptr() + 2), pk(out=out.data_ptr() + 4)] == [UNAL] * 4
    torch.cuda.synchronize()
    assert bool((out == 0xFF).all()) and int(flag.item()) == 0


# ---- 7. the operator's routes ---------------------------------------------------------------------------------------------------------------
def test_operator_routes_and_fallbacks_equal_the_unfused_graph(nv):
    pn = native()
    M, N, K, bs = 6, 40, 256, 64
    codes, s, z, qmin, qmax, nbits = real_problem("int4", N, K, bs, seed=4, all_codes=False)
    x = torch.randn(2, 3, K, generator=torch.Generator().manual_seed(8)).to(BF16).cuda()
    bias = torch.randn(N, generator=torch.Generator().manual_seed(9)).to(BF16).cuda()
    unfused = F.linear(x, dequantize_op(codes, s, z, bs), bias)
    packed = pack(nv, codes, qmin, qmax, nbits)
    op = torch.ops.quantized_ops.linear_gwa
    pn.GWA_STATS.reset()
    y = op(x, packed, s, z, bias, bs, qmin, nbits, K)                            # the rule: M = 6 takes the fused kernel
    assert (pn.GWA_STATS.fused, pn.GWA_STATS.dequant, pn.GWA_STATS.reference) == (1, 0, 0) and y.shape == (2, 3, N)
    y64 = x.double() @ dequantize_op(codes, s, z, bs).double().t() + bias.double()
    S = x.double().abs() @ dequantize_op(codes, s, z, bs).double().abs().t() + bias.double().abs()
    assert bool(((y.double() - y64).abs() <= bound_of(y64, S, K)).all())
    for route in ("dequant", "reference"):                                       # both ARE the unfused graph's arithmetic
        got = pn.linear_gwa_route(x, packed, s, z, bias, bs, qmin, nbits, K, route=route)
        assert torch.equal(bits(got), bits(unfused)), route
    assert (pn.GWA_STATS.dequant, pn.GWA_STATS.reference) == (1, 1)
    # a shape the rule leaves to the dequantize kernel + library GEMM
    big = torch.randn(pn._GWA_FUSED_MAX_M + 1, K, generator=torch.Generator().manual_seed(3)).to(BF16).cuda()
    pn.GWA_STATS.reset()
    got = op(big, packed, s, z, bias, bs, qmin, nbits, K)
    assert pn.GWA_STATS.dequant == 1 and pn.GWA_STATS.reasons == {"route rule": 1}
    assert torch.equal(bits(got), bits(F.linear(big, dequantize_op(codes, s, z, bs), bias)))
    # a shape the kernels decline: a block size of 16
    codes16, s16, z16, *_ = real_problem("int4", N, 64, 32, seed=6, all_codes=False)
    s16, z16 = s16.repeat_interleave(2, -1).contiguous(), z16.repeat_interleave(2, -1).contiguous()
    p16 = pn.gwa_pack_torch(codes16.cpu(), qmin, qmax, nbits).cuda()
    x16 = torch.randn(5, 64, generator=torch.Generator().manual_seed(2)).to(BF16).cuda()
    pn.GWA_STATS.reset()
    got = op(x16, p16, s16, z16, None, 16, qmin, nbits, 64)
    assert pn.GWA_STATS.reference == 1 and pn.GWA_STATS.fused == 0
    assert torch.equal(bits(got), bits(F.linear(x16, dequantize_op(codes16, s16, z16, 16))))


# ---- 8. a converted model -------------------------------------------------------------------------------------------------------------------
def test_converted_model_takes_the_fused_route_and_the_switch_turns_it_off(nv, monkeypatch):
    from quantized_training import fused as fz
    pn = native()
    plain, x = converted(False)
    fused_gm, _ = converted(None)                                                # the default on a device model
    assert targets(fused_gm).count(GWA) == 2 and DQ not in targets(fused_gm) and LIN not in targets(fused_gm)
    bufs = dict(fused_gm.named_buffers())
    assert sum(k.endswith("_packed") for k in bufs) == 2 and not any(k.endswith("_uint4") for k in bufs)
    assert all(v.device.type == "cuda" for v in bufs.values())
    pn.GWA_STATS.reset()
    pn.GWA_ROUTES.clear()
    with torch.no_grad():
        y, yp = fused_gm(x), plain(x)
    assert (pn.GWA_STATS.fused, pn.GWA_STATS.dequant, pn.GWA_STATS.reference) == (2, 0, 0)
    report = fz.routes_report()
    assert report.get("gwa:4x512x256") == "fused_gwa_gemm" and report.get("gwa:4x136x512") == "fused_gwa_gemm"
    # both models within the tolerance tier of the fp64 chain: layer 1's bound b1 reaches layer 2 through |Wd2|
    pb = dict(plain.named_buffers())
    dq = [n for n in plain.graph.nodes if str(n.target) == DQ]
    w1, w2 = (dequantize_op(*(pb[a.target] for a in n.args[:3]), 128).double() for n in dq)
    b1 = dict(plain.named_parameters())
    bias1 = next(v for k, v in list(b1.items()) + list(pb.items()) if v.shape == (512,) and v.dtype == BF16).double()
    h64 = x.double() @ w1.t() + bias1
    bound1 = bound_of(h64, x.double().abs() @ w1.abs().t() + bias1.abs(), 256)
    r64 = torch.relu(h64)
    y64 = r64 @ w2.t()
    tol = bound_of(y64, (r64 + bound1) @ w2.abs().t(), 512) + 1.01 * (bound1 @ w2.abs().t())
    for got in (y, yp):
        assert bool(((got.double() - y64).abs() <= tol).all()), float(((got.double() - y64).abs() / tol).max())
    # QT_PT2E_NATIVE=0: upstream's graph
    monkeypatch.setenv("QT_PT2E_NATIVE", "0")
    off, _ = converted(None)
    assert rows(off) == rows(plain)
