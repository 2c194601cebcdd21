"""The block-scaled GEMM for integer and codebook operands (qt_mxi_pack / qt_mxi_gemm, csrc/qt_mxi_gemm.hip) and its route through
linear_mx / matmul_mx (quantized_training/mx_gemm.py).

    C[b][m][n] = rd( bias[n] + sum_kb (sA[b][m][kb] sB[b][n][kb]) * p_kb ),     p_kb = sum over block kb of a[b][m][k] b[b][n][k]

p_kb is exact in int32 and in fp32 (|p_kb| <= 128 * 128 * 128 < 2^24); t_kb = fl(sA sB) is one fp32 product; acc = fma(p_kb, t_kb, acc)
in increasing kb; the bias is added in fp32 and the result rounded once.

Exact tier: power-of-two scales whose exponents span at most 2 per operand, so every term p_kb t_kb is a multiple of the quantum
q = min sA * min sB; the test asserts sum_kb |p_kb t_kb| + |bias| < 2^24 q for every output, so every partial sum of the kernel's
chain is an fp32 number and the result must be the fp64 value rounded once to the output dtype, bit for bit.

Tolerance tier (derived, not measured): with u = 2^-24, t_kb carries one rounding (|delta| <= u, none for bf16 scales, whose
product is exact in fp32), each of the nblk fmas rounds a partial sum that is bounded by S = sum_kb |term_kb| (+ |bias|), the bias
add rounds once more, and the output dtype once (unit roundoff u_out = 2^-8 for bf16's 8 significant bits, 2^-24 for fp32):
    |y - y64| <= u_out |y64| + (nblk + c) u S,       c = 3: the scale product, the bias add, and one unit for the second-order terms
(among them the output rounding acting on the accumulation error: u_out (nblk + 2) u S <= u S).
"""
import pytest
import torch
import torch.nn.functional as F

from kernel_launch import Guarded, nv, stream  # noqa: F401

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="f32")]
SHAPES = [(1, 1, 64), (16, 16, 128), (130, 136, 192), (257, 72, 320)]         # M x N x K
U = 2.0 ** -24


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def ptr(t):
    return t.data_ptr() if t is not None else None


def k_for(K, bs):
    """The issue's K where the block size divides it; for 128-blocks the next multiple of 128 (K % bs == 0 is the kernel's rule)."""
    return K if K % bs == 0 else (K + bs - 1) // bs * bs


def run_gemm(nv, a, sa, b, sb, bs, out_dtype, bias, batch, M, N, K, a_rows, b_rows, out=None):
    """qt_mxi_gemm through the C ABI.  a / b: int8 [.., K] device tensors, sa / sb: fp32; batch strides in rows."""
    c = torch.full((batch, M, N), float("nan"), dtype=out_dtype, device="cuda") if out is None else None
    rc = nv.lib().qt_mxi_gemm(a.data_ptr(), sa.data_ptr(), b.data_ptr(), sb.data_ptr(), bs, c.data_ptr() if out is None else out,
                              int(out_dtype == F32), ptr(bias), batch, M, N, K, a_rows, b_rows, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return c


def block_terms(a, sa, b, sb, bs):
    """(y64, S): the fp64 sum of the terms p_kb sA sB and the sum of their magnitudes, [batch, M, N]."""
    nb = a.shape[-1] // bs
    y = torch.zeros(a.shape[:-1] + (b.shape[-2],), dtype=torch.float64, device=a.device)
    s = torch.zeros_like(y)
    for kb in range(nb):
        p = a[..., kb * bs:(kb + 1) * bs].double() @ b[..., kb * bs:(kb + 1) * bs].double().transpose(-1, -2)
        t = p * sa[..., kb].double().unsqueeze(-1) * sb[..., kb].double().unsqueeze(-2)
        y += t
        s += t.abs()
    return y, s


# ---- 1. exact tier ------------------------------------------------------------------------------------------------------------------------
def exact_problem(M, N, K, bs, batch, seed):
    """Codes over the full int8 range (-128, -127 and 127 forced in), scales 2^e with e in [-2, 0] (A) and [0, 2] (B): q = 2^-2.  With
    batch > 1 the operands have padding rows between the batches (batch strides M + 5 and N + 3 rows)."""
    g = torch.Generator().manual_seed(seed)
    ra, rb = (M + 5, N + 3) if batch > 1 else (M, N)
    a = torch.randint(-128, 128, (batch, ra, K), generator=g, dtype=torch.int8)
    b = torch.randint(-128, 128, (batch, rb, K), generator=g, dtype=torch.int8)
    a[:, 0, 0], a[:, 0, K - 1], a[:, M - 1, 1] = -128, 127, -127
    b[:, 0, 0], b[:, 0, K - 1], b[:, N - 1, 1] = -128, -127, 127
    sa = 2.0 ** torch.randint(-2, 1, (batch, ra, K // bs), generator=g).float()
    sb = 2.0 ** torch.randint(0, 3, (batch, rb, K // bs), generator=g).float()
    bias = torch.randint(-100, 101, (N,), generator=g).float() * 0.25
    return [t.cuda() for t in (a, sa, b, sb, bias)] + [ra, rb]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("bs", [32, 64, 128])
def test_exact_tier_is_the_fp64_product_rounded_once(nv, bs, shape):
    M, N, K = shape[0], shape[1], k_for(shape[2], bs)
    for batch in (1, 3):
        a, sa, b, sb, bias, ra, rb = exact_problem(M, N, K, bs, batch, seed=M + bs + batch)
        y64, S = block_terms(a[:, :M], sa[:, :M], b[:, :N], sb[:, :N], bs)
        assert float((S + bias.abs().double()).max()) < 2.0 ** 24 * 0.25, "the data do not keep every partial sum an fp32 number"
        assert not torch.equal(y64, y64.transpose(-1, -2)) if M == N and M > 1 else True          # an asymmetric problem
        for out_dtype in (BF16, F32):
            for use_bias in (False, True):
                bv = bias.to(out_dtype) if use_bias else None
                want = (y64 + (bv.double() if use_bias else 0.0)).to(F32).to(out_dtype)
                got = run_gemm(nv, a, sa, b, sb, bs, out_dtype, bv, batch, M, N, K, ra if batch > 1 else 0, rb if batch > 1 else 0)
                assert torch.equal(bits(got), bits(want)), \
                    f"bs {bs}, {M}x{N}x{K}, batch {batch}, {out_dtype}, bias {use_bias}: {int((bits(got) != bits(want)).sum())} elements differ"


@pytest.mark.parametrize("bs", [32, 64, 128])
def test_shared_second_operand_and_two_launches(nv, bs):
    """Batch stride 0: one B for every batch; and the same bits on a second launch."""
    M, N, K = 130, 136, k_for(192, bs)
    a, sa, b, sb, bias, ra, rb = exact_problem(M, N, K, bs, 3, seed=7)
    y64, _ = block_terms(a[:, :M], sa[:, :M], b[:1, :N], sb[:1, :N], bs)
    got = run_gemm(nv, a, sa, b, sb, bs, F32, None, 3, M, N, K, ra, 0)
    assert torch.equal(bits(got), bits(y64.to(F32)))
    assert torch.equal(bits(run_gemm(nv, a, sa, b, sb, bs, F32, None, 3, M, N, K, ra, 0)), bits(got))


# ---- 2. the lane map ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [32, 64, 128])
def test_one_hot_rows_pick_the_elements_of_an_asymmetric_b(nv, bs):
    """A = one 1 per row, at k = perm(m): C[m][n] must be B[n][perm(m)], bit for bit, for every k of the tile -- the check the 32-deep
    instruction's operand lane map needs (a wrong k assignment, or rows and columns swapped, selects other elements of B)."""
    M = K = 256
    N = 80
    perm = (torch.arange(M) * 37 + 11) % K                                          # a bijection: gcd(37, 256) = 1
    a = torch.zeros(1, M, K, dtype=torch.int8)
    a[0, torch.arange(M), perm] = 1
    n, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    b = (((n * 7 + k * 13 + (n * k) % 5) % 251) - 125).to(torch.int8).unsqueeze(0)
    ones_a, ones_b = torch.ones(1, M, K // bs), torch.ones(1, N, K // bs)
    got = run_gemm(nv, a.cuda(), ones_a.cuda(), b.cuda(), ones_b.cuda(), bs, F32, None, 1, M, N, K, 0, 0)
    want = b[0].float().t()[perm]                                                    # [M, N]
    assert torch.equal(got[0].cpu(), want), f"{int((got[0].cpu() != want).sum())} of {M * N} elements"


# ---- 3. tolerance tier --------------------------------------------------------------------------------------------------------------------
def e5m3(t):
    from quantized_training.fake_quantize import get_quantization_map
    return torch.ops.quantized_ops.vmap(t.to(BF16), get_quantization_map("fp8_e5m3", t.device)).to(t.dtype)


def tolerance_problem(M, N, K, bs, dtype, kind, seed):
    """int8 codes and block scales in `dtype`: amax / qmax of normal data, as they are or rounded to fp8_e5m3."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-127, 128, (1, M, K), generator=g, dtype=torch.int8).cuda()
    b = torch.randint(-127, 128, (1, N, K), generator=g, dtype=torch.int8).cuda()
    sa = (torch.randn(1, M, K // bs, generator=g).abs() * 3 + 0.01).div(127.0).to(dtype).cuda()
    sb = (torch.randn(1, N, K // bs, generator=g).abs() * 0.5 + 0.01).div(127.0).to(dtype).cuda()
    if kind == "fp8_e5m3":
        sa, sb = e5m3(sa), e5m3(sb)
    bias = torch.randn(N, generator=g).to(dtype).cuda()
    return a, sa, b, sb, bias


def bound_of(y64, S, nblk, dtype):
    u_out = 2.0 ** -8 if dtype == BF16 else U
    return u_out * y64.abs() + (nblk + 3) * U * S + 1e-300


@pytest.mark.parametrize("kind", ["fp8_e5m3", "amax"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", [32, 64, 128])
def test_tolerance_tier_against_fp64_and_the_composite(nv, bs, dtype, kind):
    """The module docstring's bound; in bf16 the native error must not exceed that of the composite on the same operands (which rounds
    every dequantized element to bf16 before a bf16 GEMM)."""
    M, N, K = 130, 136, k_for(320, bs)
    a, sa, b, sb, bias = tolerance_problem(M, N, K, bs, dtype, kind, seed=bs + len(kind))
    y64, S = block_terms(a, sa, b, sb, bs)
    y64, S = y64 + bias.double(), S + bias.abs().double()
    got = run_gemm(nv, a, sa.float(), b, sb.float(), bs, dtype, bias, 1, M, N, K, 0, 0)
    err = (got.double() - y64).abs()
    bound = bound_of(y64, S, K // bs, dtype)
    print(f"\n[mxi_gemm bs {bs} {dtype} {kind}] largest error {float(err.max()):.3e}, largest error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements outside the bound, worst ratio {float((err / bound).max())}"
    if dtype == BF16:
        comp = F.linear(a[0].to(dtype) * sa[0].repeat_interleave(bs, -1), b[0].to(dtype) * sb[0].repeat_interleave(bs, -1), bias)
        cerr = (comp.double() - y64[0]).abs()
        print(f"[mxi_gemm bs {bs} {dtype} {kind}] composite's largest error {float(cerr.max()):.3e}")
        assert float(err.max()) <= float(cerr.max())


# ---- 4. the packer ------------------------------------------------------------------------------------------------------------------------
def nf4_6_levels(dtype):
    from quantized_training.normal_float import quantize_to_nf
    return quantize_to_nf(torch.zeros(1, dtype=dtype), 4, int_bits=6)[1]


def run_pack(nv, x, s, code, bs, batch, rows, K, xs, ss, check=True, outs=None):
    """-> (rc, codes int8 [batch, rows, K], scales fp32 [batch, rows, K / bs], flag or None)"""
    codes = torch.full((batch, rows, K), 99, dtype=torch.int8, device="cuda")
    scales = torch.full((batch, rows, K // bs), float("nan"), dtype=F32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda") if check else None
    cp, sp = (codes.data_ptr(), scales.data_ptr()) if outs is None else outs
    rc = nv.lib().qt_mxi_pack(x.data_ptr(), s.data_ptr(), int(x.dtype == F32), ptr(code), code.numel() if code is not None else 0, cp, sp,
                              batch, rows, K, *xs, *ss, bs, ptr(bad), stream())
    torch.cuda.synchronize()
    return rc, codes, scales, (int(bad.item()) if check else None)


def restated_pack(x, s, code):
    """x [batch, rows, K] logical, s [batch, rows, K / bs]: what the composite multiplies, as int8 codes and fp32 scales."""
    v = code[x.to(torch.long)] if code is not None else x
    return v.double().clamp(-128, 127).to(torch.int8), s.float()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", [32, 64, 128])
def test_pack_equals_its_restatement(nv, bs, dtype):
    g = torch.Generator().manual_seed(bs)
    rows, K, B, N = 37, 256, 3, 24
    nb = K // bs
    x = torch.randint(-128, 128, (rows, K), generator=g).to(dtype).cuda()
    s = (torch.rand(rows, nb, generator=g) + 0.01).to(dtype).cuda()
    rc, codes, scales, flag = run_pack(nv, x, s, None, bs, 1, rows, K, (0, K, 1), (0, nb, 1))
    wc, ws = restated_pack(x[None], s[None], None)
    assert (rc, flag) == (0, 0) and torch.equal(codes, wc) and torch.equal(scales.view(torch.int32), ws.view(torch.int32)), "rows"
    # the [batch N, K] second operand of matmul_mx from a [batch, K, N] tensor with [batch, K / bs, N] scales
    xb = torch.randint(-32, 32, (B, K, N), generator=g).to(dtype).cuda()
    sb = (torch.rand(B, nb, N, generator=g) + 0.01).to(dtype).cuda()
    rc, codes, scales, flag = run_pack(nv, xb, sb, None, bs, B, N, K, (K * N, 1, N), (nb * N, 1, N))
    wc, ws = restated_pack(xb.transpose(1, 2), sb.transpose(1, 2), None)
    assert (rc, flag) == (0, 0) and torch.equal(codes, wc) and torch.equal(scales.view(torch.int32), ws.contiguous().view(torch.int32)), "second operand"
    # indices into the 16 integer levels of nf4_6, whole and fractional (truncated toward zero, as .to(torch.long) does)
    code = nf4_6_levels(dtype).cuda()
    assert code.numel() == 16 and bool((code == code.round()).all())
    idx = torch.randint(0, 16, (rows, K), generator=g).to(dtype).cuda()
    frac = idx + 0.75 if dtype == F32 else idx + 0.5
    low = -frac.clamp(max=0.75)                                                      # (-1, 0]: truncates to index 0
    for what, xi in (("whole", idx), ("fractional", frac), ("just below zero", low)):
        rc, codes, scales, flag = run_pack(nv, xi, s, code, bs, 1, rows, K, (0, K, 1), (0, nb, 1))
        wc, _ = restated_pack(xi[None], s[None], code)
        assert (rc, flag) == (0, 0) and torch.equal(codes, wc), what


BAD_VALUES = [("127.5", 127.5), ("128", 128.0), ("-129", -129.0), ("nan", float("nan"))]
BAD_SCALES = [("0", 0.0), ("inf", float("inf")), ("nan", float("nan")), ("negative", -1.0)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_check_flag_and_safety_without_it(nv, dtype):
    g = torch.Generator().manual_seed(1)
    rows, K, bs = 9, 64, 32
    x0 = torch.randint(-128, 128, (rows, K), generator=g).to(dtype).cuda()
    s0 = (torch.rand(rows, 2, generator=g) + 0.5).to(dtype).cuda()
    code = nf4_6_levels(dtype).cuda()
    idx0 = torch.randint(0, 16, (rows, K), generator=g).to(dtype).cuda()
    cases = [("clean values", x0, s0, None, 0), ("clean indices", idx0, s0, code, 0)]
    for label, v in BAD_VALUES:
        x = x0.clone(); x[4, 37] = v
        cases.append((f"value {label}", x, s0, None, 1))
    for label, v in BAD_SCALES:
        s = s0.clone(); s[5, 1] = v
        cases.append((f"scale {label}", x0, s, None, 1))
    for label, v in (("an index equal to the codebook's length", 16.0), ("index -1", -1.0), ("index inf", float("inf"))):
        x = idx0.clone(); x[2, 3] = v
        cases.append((label, x, s0, code, 1))
    frac_code = code.clone(); frac_code[3] = 0.5
    cases.append(("a codebook entry that is no integer", idx0, s0, frac_code, 1))
    for label, x, s, c, want in cases:
        rc, codes, scales, flag = run_pack(nv, x, s, c, bs, 1, rows, K, (0, K, 1), (0, 2, 1))
        assert (rc, flag) == (0, want), label
        # without the flag: every output element written, nothing outside them, indices clamped and values saturated
        gc, gs = Guarded((rows, K), "int8"), Guarded((rows, 2), "float32")
        rc, _, _, _ = run_pack(nv, x, s, c, bs, 1, rows, K, (0, K, 1), (0, 2, 1), check=False, outs=(gc.ptr, gs.ptr))
        assert rc == 0 and gc.intact() and gs.intact(), label
        assert torch.equal(torch.from_numpy(gc.host()), codes.cpu()[0]), label
        if want == 0:
            wc, _ = restated_pack(x[None], s[None], c)
            assert torch.equal(codes, wc), label
    x = x0.clone(); x[0, 0], x[0, 1], x[0, 2] = 300.0, -300.0, float("nan")
    _, codes, _, flag = run_pack(nv, x, s0, None, bs, 1, rows, K, (0, K, 1), (0, 2, 1))
    assert flag == 1 and codes[0, 0, :3].tolist() == [127, -128, 0]


# ---- 5. guards ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [32, 64, 128])
def test_nothing_outside_the_operands_is_read_or_written(nv, bs):
    """Every operand sits between 0xFF code bytes / NaN scales: a read outside would reach the (exact-tier) result."""
    M, N, K = 130, 136, k_for(192, bs)
    a, sa, b, sb, bias, _, _ = exact_problem(M, N, K, bs, 1, seed=3)
    y64, _ = block_terms(a, sa, b, sb, bs)
    PAD = 4096

    def fenced(t, fill):
        raw = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device="cuda")
        raw[PAD:PAD + t.numel()] = t.reshape(-1)
        return raw, raw[PAD:PAD + t.numel()]
    ra, va = fenced(a, -1)
    rb, vb = fenced(b, -1)
    rsa, vsa = fenced(sa, float("nan"))
    rsb, vsb = fenced(sb, float("nan"))
    before = [r.clone() for r in (ra, rb, rsa, rsb)]
    for out_dtype, np_dtype in ((F32, "float32"), (BF16, "uint16")):
        out = Guarded((1, M, N), np_dtype)
        run_gemm(nv, va, vsa, vb, vsb, bs, out_dtype, None, 1, M, N, K, 0, 0, out=out.ptr)
        assert out.intact()
        got = torch.from_numpy(out.host().view("int32" if out_dtype == F32 else "int16"))
        assert torch.equal(got, bits(y64.to(F32).to(out_dtype)).cpu())
    for r, r0 in zip((ra, rb, rsa, rsb), before):
        assert torch.equal(r.view(torch.uint8), r0.view(torch.uint8))


# ---- 6. the operators ---------------------------------------------------------------------------------------------------------------------
def qmap_of(name):
    from quantized_training.fake_quantize import get_quantization_map
    return get_quantization_map(name, "cuda")


def quantized(x, fmt, bs, axis, scale_fmt=None, pow2=False):
    """(values or indices, block scales, codebook or None) through the engine's own quantize_mx."""
    from quantized_training.quantizer.quantizer import get_quant_min_max
    qmap, code = qmap_of(fmt), None
    if isinstance(qmap, tuple):
        qmap, code = qmap[0], qmap[1].to(x.dtype)
    s, q = torch.ops.quantized_ops.quantize_mx(x, qmap, [axis], bs, float(get_quant_min_max(fmt)[1]), pow2,
                                               qmap_of(scale_fmt) if scale_fmt else None, None)
    return q, s, code


def lookup64(q, code):
    return (code[q.to(torch.long)] if code is not None else q).double()


def stats():
    from quantized_training import mx_gemm
    return mx_gemm.STATS.native, mx_gemm.STATS.fallback


def reset():
    from quantized_training import mx_gemm
    mx_gemm.STATS.reset()


def composite_linear(x, w, bias, sx, sw, bs, xc, wc):
    """decomposed.py's composite restated: codebook lookup, scales repeated over their blocks, F.linear."""
    dx = (xc[x.to(torch.long)].to(x.dtype) if xc is not None else x) * sx.repeat_interleave(bs, -1)
    dw = (wc[w.to(torch.long)].to(w.dtype) if wc is not None else w) * sw.repeat_interleave(bs, -1)
    return F.linear(dx, dw, bias)


def composite_matmul(a, b, sa, sb, bs, ac, bc):
    da = (ac[a.to(torch.long)].to(a.dtype) if ac is not None else a) * sa.repeat_interleave(bs, -1)
    db = (bc[b.to(torch.long)].to(b.dtype) if bc is not None else b) * sb.repeat_interleave(bs, -2)
    return torch.matmul(da, db)


def linear_mx(x, w, bias, sx, sw, bs, xc=None, wc=None):
    return torch.ops.quantized_ops.linear_mx(x, w, bias, input_scale=sx, weight_scale=sw, block_size=bs, input_code=xc, weight_code=wc)


def matmul_mx(a, b, sa, sb, bs, ac=None, bc=None):
    return torch.ops.quantized_ops.matmul_mx(a, b, input_scale=sa, weight_scale=sb, block_size=bs, input_code=ac, weight_code=bc)


LINEAR_CONFIGS = {      # name -> (input format, weight format, block size, scale format)
    "int8_bs32": ("int8", "int8", 32, None),
    "int6_bs64_e5m3": ("int6", "int6", 64, "fp8_e5m3"),
    "int8_x_nf4_6": ("int8", "nf4_6", 64, "fp8_e5m3"),
    "nf4_6_x_int6": ("nf4_6", "int6", 64, "fp8_e5m3"),
    "nf4_6_both": ("nf4_6", "nf4_6", 64, "fp8_e5m3"),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(LINEAR_CONFIGS))
def test_linear_mx_takes_the_integer_route(nv, name, dtype):
    fx, fw, bs, sf = LINEAR_CONFIGS[name]
    g = torch.Generator().manual_seed(11)
    x0 = (torch.randn(3, 50, 192, generator=g) * 2).to(dtype).cuda()
    w0 = (torch.randn(72, 192, generator=g) * 0.3).to(dtype).cuda()
    bias = torch.randn(72, generator=g).to(dtype).cuda()
    (x, sx, xc), (w, sw, wc) = quantized(x0, fx, bs, -1, sf), quantized(w0, fw, bs, -1, sf)
    reset()
    y = linear_mx(x, w, bias, sx, sw, bs, xc, wc)
    assert stats() == (1, 0) and y.shape == (3, 50, 72) and y.dtype == dtype
    a, b = lookup64(x, xc).reshape(1, 150, 192), lookup64(w, wc).reshape(1, 72, 192)
    y64, S = block_terms(a, sx.reshape(1, 150, -1), b, sw.reshape(1, 72, -1), bs)
    y64, S = y64 + bias.double(), S + bias.abs().double()
    err = (y.double().reshape(1, 150, 72) - y64).abs()
    bound = bound_of(y64, S, 192 // bs, dtype)
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["int6 ax=-2", "int6 transposed view", "int8 bs=32", "nf4_6 both"])
def test_matmul_mx_takes_the_integer_route(nv, case, dtype):
    g = torch.Generator().manual_seed(12)
    B, M, K, N = 3, 70, 128, 40
    fmt, bs, sf = {"int6 ax=-2": ("int6", 64, "fp8_e5m3"), "int6 transposed view": ("int6", 64, "fp8_e5m3"), "int8 bs=32": ("int8", 32, None),
                   "nf4_6 both": ("nf4_6", 64, "fp8_e5m3")}[case]
    a0 = torch.randn(B, M, K, generator=g).to(dtype).cuda()
    if case == "int6 transposed view":                              # Q . K^T: the second operand is a transposed view of [B, N, K]
        b0 = torch.randn(B, N, K, generator=g).to(dtype).cuda().transpose(-1, -2)
    else:
        b0 = torch.randn(B, K, N, generator=g).to(dtype).cuda()
    (a, sa, ac), (b, sb, bc) = quantized(a0, fmt, bs, -1, sf), quantized(b0, fmt, bs, -2, sf)
    reset()
    y = matmul_mx(a, b, sa, sb, bs, ac, bc)
    assert stats() == (1, 0) and y.shape == (B, M, N) and y.dtype == dtype
    y64, S = block_terms(lookup64(a, ac), sa, lookup64(b, bc).transpose(-1, -2), sb.transpose(-1, -2), bs)
    err = (y.double() - y64).abs()
    bound = bound_of(y64, S, K // bs, dtype)
    assert bool((err <= bound).all()), float((err / bound).max())


def int8_linear_problem(dtype=BF16, bs=32, K=128):
    g = torch.Generator().manual_seed(13)
    x0, w0 = (torch.randn(40, K, generator=g) * 2).to(dtype).cuda(), (torch.randn(24, K, generator=g) * 0.3).to(dtype).cuda()
    (x, sx, _), (w, sw, _) = quantized(x0, "int8", bs, -1), quantized(w0, "int8", bs, -1)
    return dict(x=x, w=w, bias=None, sx=sx, sw=sw, bs=bs, xc=None, wc=None)


def _float_input(p):
    p["x"], p["sx"], _ = quantized(p["x"] * p["sx"].repeat_interleave(32, -1), "fp8_e4m3", 32, -1, pow2=True)


def _float_weight(p):
    w, sw, _ = quantized(p["w"] * p["sw"].repeat_interleave(32, -1), "fp8_e4m3", 32, -1)          # amax scales: the float packer refuses them
    p["w"], p["sw"] = w, sw


def _nf4_levels(p):
    q, s, code = quantized(torch.randn(24, 128, device="cuda").to(BF16), "nf4", 32, -1)
    assert not bool((code == code.round()).all())
    p["w"], p["sw"], p["wc"] = q, s, code


def _block(bs):
    def change(p):
        p.update(int8_linear_problem(bs=bs, K=512))
    return change


def _fp16(p):
    for k in ("x", "w", "sx", "sw"):
        p[k] = p[k].half()


def _big_codebook(p):
    p["wc"] = torch.arange(-128, 129, device="cuda").to(BF16).clamp(max=127)          # 257 entries
    p["w"] = p["w"] + 128


def _no_record(p):
    p["x"] = p["x"].clone()


def _scale_shape(p):
    p["sx"] = p["sx"][:, :2].contiguous()


def _fractional_weight(p):
    from quantized_training import mx_operand
    p["w"] = mx_operand.set_format(p["w"] + 0.5, "int8")            # the record lies: the packer's check refuses the weight


DECLINES = [("a float input with an integer weight", _float_input), ("an integer input with a float weight", _float_weight),
            ("nf4 levels that are no integers", _nf4_levels), ("block size 16", _block(16)), ("block size 256", _block(256)), ("fp16", _fp16),
            ("a codebook of 257 entries", _big_codebook), ("an integer activation without record or codebook", _no_record),
            ("a weight the packer's check refuses", _fractional_weight)]


@pytest.mark.parametrize("change", [pytest.param(c, id=label) for label, c in DECLINES])
def test_declines_run_the_composite_and_count_it(nv, change):
    p = int8_linear_problem()
    reset()
    linear_mx(**p)
    assert stats() == (1, 0), "the untouched call"
    change(p)
    reset()
    y = linear_mx(**p)
    want = composite_linear(**p)
    assert stats() == (0, 1)
    assert y.dtype == want.dtype and torch.equal(y.view(torch.int16), want.view(torch.int16))


def test_the_route_rule_keeps_a_large_bf16_problem_with_the_composite(nv):
    """profiles/mx_int_gemm.txt: bf16 above 2^29 multiply-adds is the library GEMM's; the same problem in fp32 goes native."""
    g = torch.Generator().manual_seed(17)
    for dtype, want in ((BF16, (0, 1)), (F32, (1, 0))):
        x0, w0 = (torch.randn(1024, 512, generator=g) * 2).to(dtype).cuda(), (torch.randn(2048, 512, generator=g) * 0.3).to(dtype).cuda()
        (x, sx, _), (w, sw, _) = quantized(x0, "int8", 32, -1), quantized(w0, "int8", 32, -1)
        reset()
        y = linear_mx(x, w, None, sx, sw, 32)
        assert stats() == want
        if dtype == BF16:
            assert torch.equal(bits(y), bits(composite_linear(x, w, None, sx, sw, 32, None, None)))


def test_a_wrong_scale_shape_declines(nv):
    p = int8_linear_problem()
    _scale_shape(p)
    reset()
    with pytest.raises(RuntimeError):                               # the composite cannot broadcast it either
        linear_mx(**p)
    assert stats() == (0, 1)


def test_cpu_tensors_and_the_switch(nv, monkeypatch):
    p = int8_linear_problem()
    reset()
    linear_mx(**p)
    cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in p.items()}
    yc = linear_mx(**cpu)
    assert stats() == (1, 0) and torch.equal(yc.view(torch.int16), composite_linear(**cpu).view(torch.int16))
    monkeypatch.setenv("QT_MX_GEMM", "0")
    reset()
    off = linear_mx(**p)
    assert stats() == (0, 0) and torch.equal(off.view(torch.int16), composite_linear(**p).view(torch.int16))
    a, b = quantized(torch.randn(2, 40, 64, device="cuda").to(BF16), "int6", 64, -1), quantized(torch.randn(2, 64, 24, device="cuda").to(BF16), "int6", 64, -2)
    off = matmul_mx(a[0], b[0], a[1], b[1], 64)
    assert stats() == (0, 0) and torch.equal(off.view(torch.int16), composite_matmul(a[0], b[0], a[1], b[1], 64, None, None).view(torch.int16))


@pytest.mark.parametrize("write", ["scale", "codebook indices"])
def test_a_written_to_weight_is_packed_again(nv, write):
    """The cache key carries the version counters: the call stays native and multiplies the new contents."""
    g = torch.Generator().manual_seed(14)
    x0, w0 = (torch.randn(40, 128, generator=g) * 2).to(BF16).cuda(), (torch.randn(24, 128, generator=g) * 0.3).to(BF16).cuda()
    fw = "int8" if write == "scale" else "nf4_6"

    def fresh():
        (x, sx, _), (w, sw, wc) = quantized(x0, "int8", 64, -1), quantized(w0, fw, 64, -1)
        return dict(x=x, w=w, bias=None, sx=sx, sw=sw, bs=64, xc=None, wc=wc)
    p = fresh()
    y0 = linear_mx(**p)                                             # the weight's operand is cached now
    if write == "scale":
        p["sw"].mul_(2)
    else:
        p["w"].copy_(15 - p["w"])
    reset()
    y = linear_mx(**p)
    assert stats() == (1, 0)
    q = fresh()
    if write == "scale":
        q["sw"] = q["sw"] * 2
    else:
        q["w"] = 15 - q["w"]
    want = linear_mx(**q)
    assert stats() == (2, 0)
    assert torch.equal(y.view(torch.int16), want.view(torch.int16)) and not torch.equal(y.view(torch.int16), y0.view(torch.int16))


# ---- 7. the float route is untouched ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", ["fp8_e4m3", "int4"])
def test_float_route_still_serves_its_operands(nv, weight, monkeypatch):
    """An fp8_e4m3 pair, and an int4 weight with power-of-two scales (which packs as a float format): qt_mx_gemm serves them as before
    this route existed, qt_mxi_gemm is not called."""
    L = nv.lib()
    calls = []
    for name in ("qt_mx_gemm", "qt_mxi_gemm"):
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1])
    g = torch.Generator().manual_seed(15)
    # K = 96: a 6-bit row would be 72 bytes, so the int4 weight (5 and 7 are no fp4 values) packs as fp8_e4m3
    x0, w0 = torch.randn(40, 96, generator=g).to(BF16).cuda(), torch.randn(24, 96, generator=g).to(BF16).cuda()
    (x, sx, _), (w, sw, _) = quantized(x0, "fp8_e4m3", 32, -1, pow2=True), quantized(w0, weight, 32, -1, pow2=True)
    reset()
    linear_mx(x, w, None, sx, sw, 32)
    assert stats() == (1, 0) and calls == ["qt_mx_gemm"]


# ---- 8. graph capture ---------------------------------------------------------------------------------------------------------------------
def captured(fn, static_inputs, fresh_inputs):
    """Warm-up on a side stream, capture, then replay on fresh contents: bit-equal to the eager call on those contents."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        fn(*static_inputs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = fn(*static_inputs)
    for fresh in fresh_inputs:
        for s, f in zip(static_inputs, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            want = fn(*fresh)
        assert torch.equal(bits(out), bits(want))


def test_linear_and_matmul_replay_under_graph_capture(nv):
    g = torch.Generator().manual_seed(16)
    r = lambda *s: torch.randn(*s, generator=g).to(BF16).cuda()     # noqa: E731
    w, sw, _ = quantized(r(72, 128) * 0.3, "int6", 64, -1, "fp8_e5m3")
    bias = r(72)

    def linear(x0):
        x, sx, _ = quantized(x0, "int6", 64, -1, "fp8_e5m3")
        return linear_mx(x, w, bias, sx, sw, 64)

    def matmul(a0, b0):
        (a, sa, _), (b, sb, _) = quantized(a0, "int8", 32, -1), quantized(b0, "int8", 32, -2)
        return matmul_mx(a, b, sa, sb, 32)
    reset()
    captured(linear, [r(50, 128)], [[r(50, 128)], [r(50, 128) * 3]])
    captured(matmul, [r(3, 70, 64), r(3, 64, 40)], [[r(3, 70, 64), r(3, 64, 40)]])
    assert stats()[1] == 0 and stats()[0] >= 4


def test_converted_outlier_model_runs_one_integer_gemm_per_layer(nv):
    """The two-Linear model of tests/golden/outlier.json (int8, bs = 32, outlier = 4.5): the linear_mx between filter_outlier and
    spmm_csr is native now, the result stays within the existing test's 1e-5 of the CPU graph, and the graph replays."""
    from test_gpu_outlier import converted_two_linear
    gc_cpu, x_cpu = converted_two_linear("cpu")
    gc, x = converted_two_linear("cuda")
    with torch.no_grad():
        want = gc_cpu(x_cpu)
        reset()
        y = gc(x)
    assert stats() == (2, 0)
    assert float((want - y.cpu()).abs().max()) <= 1e-5 * float(want.abs().max())
    captured(gc, [x.clone()], [[x * 0.5], [x]])
