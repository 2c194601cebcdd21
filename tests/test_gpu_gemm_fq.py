"""The fake-quant GEMM (csrc/qt_gemm.hip: qt_linear_fq_bf16, qt_bmm_fq_bf16) at every instantiation of gemm_fq_kernel<BMODE, OBS_B, B_NN>
and every run-time path behind them, through the C ABI.  Cases: tests/gemm_fq_cases.py; what they guarantee on their own (all 16
instantiations reached, exact inputs exact, room under the tolerance): tests/test_gemm_fq_cases_cpu.py.

Tier 1  the fake-quantizer the kernel applies while it stages an operand, on all 65 536 bf16 patterns, read out through an identity
        operand: bit for bit the oracle's fq_bf16 and a qt_fake_quant_bf16 launch, amax slots included.
Tier 2  tiles, tails, layouts, strides and the store paths on operands whose products and sums are exact in fp32: bit for bit the fp64
        product rounded once, guard bands intact, two launches identical; refusals write nothing.
Tier 3  general scales against the fp64 product of the oracle-quantized operands under the project's own product criterion
        (tests/test_gpu_parity.py::_products_close).

Run on the MI355X box:  python -m pytest tests/test_gpu_gemm_fq.py -m gpu -q -s
"""
import ctypes

import numpy as np
import pytest
import torch

import gemm_fq_cases as gc
from oracle import qt_oracle as o

from kernel_launch import OK, SENTINEL, Guarded, dev, launch, nv, refused, same, stream  # noqa: F401

pytestmark = pytest.mark.gpu

NAN16 = 0x7FC0
SUBNORMALS = {}                       # what Tier 1 saw of bf16-subnormal values: name -> (kept by the kernel, kept by torch.matmul, of)


def teardown_module(module):
    for k, (kern, mm, n) in sorted(SUBNORMALS.items()):
        print(f"\n[gemm_fq] {k}: bf16-subnormal quantized values kept by the kernel {kern} / by torch.matmul {mm} of {n}")


class Operand:
    """A qt_operand_q for a gc.BMode; owns the device buffers behind its pointers.  amax: None = as the mode says with a zeroed slot."""

    def __init__(self, nv, mode, table=True):
        self.mode = mode
        self.q = nv.QtOperandQ()
        self.q.fmt = nv.QtFormat(nv.QT_FMT_IDENTITY, 0, 0, 0.0, 0.0) if mode.dtype is None else nv.format_for(mode.dtype)
        assert self.q.fmt.kind == mode.kind, mode.id
        self.lut = dev(nv.build_map_u16(mode.dtype)) if mode.kind == gc.KIND_LUT and table else None
        self.scale = dev(np.array([mode.scale], np.float32)) if mode.scale is not None else None
        self.amax = torch.zeros(1, dtype=torch.int32, device="cuda") if mode.obs else None
        self.q.lut_dev = self.lut.data_ptr() if self.lut is not None else None
        self.q.scale_f32_dev = self.scale.data_ptr() if self.scale is not None else None
        self.q.amax_bits_dev = self.amax.data_ptr() if self.amax is not None else None

    @property
    def ref(self):
        return ctypes.byref(self.q)

    def fill(self, bits):
        if self.amax is not None:
            self.amax.fill_(int(np.array([bits], np.uint32).view(np.int32)[0]))

    def slot(self):
        return int(self.amax.cpu().numpy().view(np.uint32)[0])


PASS = gc.BMode(None, None, False)


def linear(nv, x, w, bias, y_ptr, M, N, K, qx, qw):
    return nv.lib().qt_linear_fq_bf16(x.data_ptr() if hasattr(x, "data_ptr") else x, w.data_ptr() if hasattr(w, "data_ptr") else w,
                                      bias.data_ptr() if bias is not None else None, y_ptr, M, N, K, qx.ref, qw.ref, stream())


def bmm(nv, a, b, y_ptr, B, M, N, K, lda, sa, ldb_k, ldb_n, sb, qa, qb):
    return nv.lib().qt_bmm_fq_bf16(a.data_ptr() if hasattr(a, "data_ptr") else a, b.data_ptr() if hasattr(b, "data_ptr") else b, y_ptr,
                                   B, M, N, K, lda, sa, ldb_k, ldb_n, sb, qa.ref, qb.ref, stream())


def fq_pass(nv, bits, mode):
    """qt_fake_quant_bf16 on a tensor under `mode` (the elementwise pass the GEMM's header names): (bits, amax slot from zero)."""
    op = Operand(nv, mode if mode.obs else gc.BMode(mode.dtype, mode.scale, True))
    lut = op.lut if op.lut is not None else None
    x = dev(bits.reshape(-1))
    y = torch.empty_like(x)
    nv.check(nv.lib().qt_fake_quant_bf16(x.data_ptr(), y.data_ptr(), x.numel(), ctypes.byref(op.q.fmt), lut.data_ptr() if lut is not None else None,
                                         op.scale.data_ptr() if op.scale is not None else None, op.amax.data_ptr(), stream()), "fq")
    torch.cuda.synchronize()
    return y.cpu().numpy().view(np.uint16).reshape(bits.shape), op.slot()


def matmul_bits(a_bits, b_bits):
    """torch.matmul on the device on bf16 operands given as bits (a [M,K], b [K,N])."""
    y = torch.matmul(dev(a_bits).view(torch.bfloat16), dev(b_bits).view(torch.bfloat16))
    return y.view(torch.int16).cpu().numpy().view(np.uint16)


def selector_expectation(name, exp):
    """What an identity operand reads out of the quantized patterns `exp` (any shape, pattern order): the oracle's value with -0 as +0;
    where that value is a bf16 subnormal, what torch.matmul gives on the device for the same product (never the kernel under test)."""
    flat = exp.reshape(gc.SEL_K, -1)                                     # as a [K, N] operand under a 128 x 128 identity
    mm = matmul_bits(gc.identity_bits(), flat).reshape(exp.shape)
    sub = gc.is_subnormal(exp)
    same(gc.pos_zero(mm), gc.pos_zero(exp), f"{name}: torch.matmul through an identity, normal values", ~sub)
    return np.where(sub, gc.pos_zero(mm), gc.pos_zero(exp)), sub, mm


def note_subnormals(name, sub, got, mm):
    if sub.any():
        SUBNORMALS[name] = (int((got[sub] & 0x7FFF != 0).sum()), int((mm[sub] & 0x7FFF != 0).sum()), int(sub.sum()))


# ---- Tier 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", gc.TIER1_B_MODES, ids=lambda m: m.id)
def test_staged_b_quantizer_on_every_pattern(nv, mode):
    """W = all 65 536 bf16 patterns as 512 x 128 (+0 where the oracle's quantized value is not finite), A = the 128 x 128 identity: y is
    fq(W) read out, whatever the accumulation order.  NT through qt_linear_fq_bf16, NT and NN through qt_bmm_fq_bf16; equal to the
    oracle's fq_bf16 and to qt_fake_quant_bf16 on the same W, -0 read as +0; the amax slot, as bits, what that pass leaves.
    bf16-subnormal quantized values: the expectation is torch.matmul's result for the same product on the device (the module's
    teardown prints the counts with -s).  Observed on the MI355X, not known beforehand: only the identity modes have such values (the
    254 subnormal patterns; every 8-bit format sends them to zero or to its smallest value), and both torch.matmul and this kernel
    keep all 254 -- the bf16 matrix instruction does not flush subnormal operands, nor does the fp32 -> bf16 rounding of the result.
    Run once on scratch copies of the kernel: without the redo block of quant_vec every case still passes (the redo cannot change a
    result on bf16 operands, tests/test_gemm_fq_cases_cpu.py); with the quotient passed on unrounded instead of as bf16 the cases
    e4m3 / int8 / uint8 at the two non-power-of-two scales fail, and no other."""
    w, exp = gc.selector_operand(mode)
    single, slot = fq_pass(nv, w, mode)
    same(single, exp, f"{mode.id}: qt_fake_quant_bf16 against the oracle")
    want, sub, mm = selector_expectation(mode.id, exp)
    eye = dev(gc.identity_bits())
    K, N = gc.SEL_K, gc.SEL_ROWS
    w_nt, w_nn = dev(w), dev(w.reshape(K, N))
    qa, qb = Operand(nv, PASS), Operand(nv, mode)
    for entry, nn in gc.ROUTES:
        what = f"{mode.id} {entry} {'NN' if nn else 'NT'} {gc.MODE_NAMES[mode.inst(nn)[0]]}"

        def go(g):
            qb.fill(0)
            if entry == "linear":
                return linear(nv, eye, w_nt, None, g["y"].ptr, K, N, K, qa, qb)
            if nn:
                return bmm(nv, eye, w_nn, g["y"].ptr, 1, K, N, K, K, K * K, N, 1, K * N, qa, qb)
            return bmm(nv, eye, w_nt, g["y"].ptr, 1, K, N, K, K, K * K, 1, K, K * N, qa, qb)

        y = launch(go, {"y": ((K, N), np.uint16)}, what)["y"]
        got = gc.pos_zero(y.reshape(K, N) if nn else y.T).reshape(exp.shape)      # NN: y = fq(W as [K, N]); NT: y[m][n] = fq(W)[n][m]
        same(got, want, what)
        same(got, gc.pos_zero(single), what + " against qt_fake_quant_bf16", ~sub)
        note_subnormals(mode.id, sub, got, mm)
        if mode.obs:
            assert qb.slot() == slot, f"{what}: amax {qb.slot():#010x}, the elementwise pass leaves {slot:#010x}"


@pytest.mark.parametrize("mode", gc.TIER1_A_MODES, ids=lambda m: m.id)
def test_staged_a_quantizer_on_every_pattern(nv, mode):
    """The mirror image: A holds the patterns as 512 x 128 and is quantized in the kernel (the generic path behind the qa lambda), B is
    the identity in pass mode, y = fq(A)."""
    a, exp = gc.selector_operand(mode)
    single, slot = fq_pass(nv, a, mode)
    same(single, exp, f"{mode.id}: qt_fake_quant_bf16 against the oracle")
    want, sub, mm = selector_expectation("A " + mode.id, exp)
    eye, ad = dev(gc.identity_bits()), dev(a)
    M, K = gc.SEL_ROWS, gc.SEL_K
    qa, qb = Operand(nv, mode), Operand(nv, PASS)
    for entry, nn in gc.ROUTES:
        what = f"A {mode.id} {entry} {'NN' if nn else 'NT'}"

        def go(g):
            qa.fill(0)
            if entry == "linear":
                return linear(nv, ad, eye, None, g["y"].ptr, M, K, K, qa, qb)
            return bmm(nv, ad, eye, g["y"].ptr, 1, M, K, K, K, M * K, K if nn else 1, 1 if nn else K, K * K, qa, qb)

        got = gc.pos_zero(launch(go, {"y": ((M, K), np.uint16)}, what)["y"])
        same(got, want, what)
        same(got, gc.pos_zero(single), what + " against qt_fake_quant_bf16", ~sub)
        note_subnormals("A " + mode.id, sub, got, mm)
        if mode.obs:
            assert qa.slot() == slot, f"{what}: amax {qa.slot():#010x}, the elementwise pass leaves {slot:#010x}"


@pytest.mark.parametrize("entry,nn", gc.ROUTES)
def test_amax_slots_only_ever_rise(nv, entry, nn):
    """A slot that already holds a larger value is unchanged, one that holds a smaller non-zero value is raised to the tensor's amax;
    both operands' slots, in launches of several workgroups."""
    M, N, K = 130, 136, 72
    c = gc.exact_operands((M, N, K), "int8", 7)
    a_mode, b_mode = gc.BMode("e4m3", None, True), c["mode"]
    want_a, want_b = int((c["a"] & 0x7FFF).max()) << 16, int((c["w"] & 0x7FFF).max()) << 16
    assert fq_pass(nv, c["a"], a_mode)[1] == want_a and fq_pass(nv, c["w"], b_mode)[1] == want_b
    a, w = dev(c["a"]), dev(np.ascontiguousarray(c["w"].T) if nn else c["w"])
    qa, qb = Operand(nv, a_mode), Operand(nv, b_mode)
    _, ref = gc.exact_product(c["a"], b_mode.fq(c["w"]))
    for fill_a, fill_b, exp_a, exp_b in ((want_a + 0x10000, want_b + 0x10000, want_a + 0x10000, want_b + 0x10000), (0x00010000, 0x00800000, want_a, want_b),
                                         (want_a, 0, want_a, want_b)):
        def go(g):
            qa.fill(fill_a)
            qb.fill(fill_b)
            if entry == "linear":
                return linear(nv, a, w, None, g["y"].ptr, M, N, K, qa, qb)
            return bmm(nv, a, w, g["y"].ptr, 1, M, N, K, K, M * K, N if nn else 1, 1 if nn else K, N * K, qa, qb)

        same(launch(go, {"y": ((M, N), np.uint16)}, f"prefilled slots {entry} nn={nn}")["y"], ref, f"prefilled slots {entry} nn={nn}")
        assert (qa.slot(), qb.slot()) == (exp_a, exp_b), (hex(fill_a), hex(fill_b), hex(qa.slot()), hex(qb.slot()))


# ---- Tier 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("which", list(gc.EXACT_MODES))
@pytest.mark.parametrize("shape", gc.EXACT_LINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_exact_tiles_and_tails(nv, shape, which, with_bias):
    """Integer A, weights that quantize to multiples of one power of two, a bias on the same grid: every product and partial sum is exact
    in fp32, so y is the fp64 product rounded once, bit for bit.  One tile, ragged M / N, K tails, N % 8 != 0 (scalar stores)."""
    M, N, K = shape
    c = gc.exact_operands(shape, which, 100 + gc.EXACT_LINEAR_SHAPES.index(shape))
    bias_bits = c["bias"] if with_bias else None
    _, ref = gc.exact_product(c["a"], c["mode"].fq(c["w"]), bias_bits)
    x, w, b = dev(c["a"]), dev(c["w"]), dev(c["bias"]) if with_bias else None
    qx, qw = Operand(nv, PASS), Operand(nv, c["mode"])

    def go(g):
        qw.fill(0)
        return linear(nv, x, w, b, g["y"].ptr, M, N, K, qx, qw)

    what = f"linear {shape} {which} bias={with_bias}"
    same(launch(go, {"y": ((M, N), np.uint16)}, what)["y"], ref, what)
    assert qw.slot() == int((c["w"] & 0x7FFF).max()) << 16, what


@pytest.mark.parametrize("which", list(gc.EXACT_MODES))
def test_linear_output_at_a_two_byte_aligned_address(nv, which):
    """y two bytes into its buffer: accepted, stored element by element; the element in front of it and those behind stay untouched."""
    shape = M, N, K = (129, 136, 72)
    c = gc.exact_operands(shape, which, 11)
    _, ref = gc.exact_product(c["a"], c["mode"].fq(c["w"]), c["bias"])
    x, w, b = dev(c["a"]), dev(c["w"]), dev(c["bias"])
    qx, qw = Operand(nv, PASS), Operand(nv, gc.BMode(c["mode"].dtype, c["mode"].scale, False))
    y = launch(lambda g: linear(nv, x, w, b, g["y"].ptr + 2, M, N, K, qx, qw), {"y": ((M * N + 8,), np.uint16)}, "misaligned y")["y"]
    pad = SENTINEL * 0x0101
    assert y[0] == pad and bool((y[1 + M * N:] == pad).all())
    same(y[1:1 + M * N].reshape(M, N), ref, f"misaligned y {which}")


def padded(bits, ld, stride, fill=NAN16):
    """[B, R, C] -> flat buffer with row stride ld and batch stride `stride`, NaN in the padding (a read of it would show in y)."""
    B, R, C = bits.shape
    out = np.full(B * stride, fill, np.uint16)
    for i in range(B):
        rows = out[i * stride:i * stride + R * ld].reshape(R, ld)
        rows[:, :C] = bits[i]
    return out


def _bmm_cases():
    for n in gc.NN_SIZES:
        for k in gc.NN_SIZES:
            yield (40, n, k), "int8", 200 + n + k
    yield (130, 136, 72), "e4m3", 300


@pytest.mark.parametrize("nn", [False, True], ids=["NT", "NN"])
@pytest.mark.parametrize("shape,which,seed", list(_bmm_cases()), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_bmm_exact_strides_and_layouts(nv, shape, which, seed, nn):
    """Batch 3 with batch strides, lda > K and a padded B (rows of K + 8 in NT, of N + 8 in NN; NaN in all padding), both operands
    quantized in the kernel (A: e4m3 at unit scale, which keeps its small integers), both observers.  NN at N and K in {8, 72, 136}:
    the n-group clamp and the K-tail row guards of the transposing stager."""
    Bn, (M, N, K) = 3, shape
    c = gc.exact_operands(shape, which, seed, Bn)
    wq = c["mode"].fq(c["w"])
    _, ref = gc.exact_product(c["a"], wq)
    lda, sa = K + 8, M * (K + 8) + 16
    a = dev(padded(c["a"], lda, sa))
    if nn:
        ldb_k, ldb_n, sb = N + 8, 1, K * (N + 8) + 8
        b = dev(padded(np.ascontiguousarray(np.swapaxes(c["w"], 1, 2)), ldb_k, sb))
    else:
        ldb_k, ldb_n, sb = 1, K + 8, N * (K + 8) + 8
        b = dev(padded(c["w"], ldb_n, sb))
    qa, qb = Operand(nv, gc.BMode("e4m3", None, True)), Operand(nv, c["mode"])

    def go(g):
        qa.fill(0)
        qb.fill(0)
        return bmm(nv, a, b, g["y"].ptr, Bn, M, N, K, lda, sa, ldb_k, ldb_n, sb, qa, qb)

    what = f"bmm {shape} {which} nn={nn}"
    same(launch(go, {"y": ((Bn, M, N), np.uint16)}, what)["y"], ref, what)
    assert qa.slot() == int((c["a"] & 0x7FFF).max()) << 16 and qb.slot() == int((c["w"] & 0x7FFF).max()) << 16, what


@pytest.mark.parametrize("nn", [False, True], ids=["NT", "NN"])
def test_bmm_shared_b_is_observed_once(nv, nn):
    """sb == 0: one B for every batch; its observer leaves what the single pass on B leaves."""
    Bn, (M, N, K) = 3, (130, 136, 72)
    c = gc.exact_operands((M, N, K), "int8", 17, Bn)
    w = c["w"][0]
    _, ref = gc.exact_product(c["a"], c["mode"].fq(w)[None])
    a, b = dev(c["a"]), dev(np.ascontiguousarray(w.T) if nn else w)
    qa, qb = Operand(nv, PASS), Operand(nv, c["mode"])

    def go(g):
        qb.fill(0)
        return bmm(nv, a, b, g["y"].ptr, Bn, M, N, K, K, M * K, N if nn else 1, 1 if nn else K, 0, qa, qb)

    same(launch(go, {"y": ((Bn, M, N), np.uint16)}, f"shared B nn={nn}")["y"], ref, f"shared B nn={nn}")
    assert qb.slot() == fq_pass(nv, w, c["mode"])[1] == int((w & 0x7FFF).max()) << 16


def test_refusals_write_nothing(nv):
    """Every argument check of both entry points, on valid buffers: an error code, y and the amax slots untouched."""
    M, N, K = 16, 16, 16
    buf = dev(np.zeros(65536 * 64 + 64, np.uint16))                      # large enough for every shape named below
    p = buf.data_ptr()
    ident, e4 = Operand(nv, PASS), Operand(nv, gc.BMode("e4m3", None, True))
    table_without_table = Operand(nv, gc.BMode("posit8_1", None, False), table=False)
    e4.fill(0x12340000)
    y = {"y": ((65536 * 8,), np.uint16)}
    lin = [("K % 8 != 0", lambda g: linear(nv, p, p, None, g["y"].ptr, M, N, 12, ident, e4)),
           ("K == 0", lambda g: linear(nv, p, p, None, g["y"].ptr, M, N, 0, ident, e4)),
           ("K < 0", lambda g: linear(nv, p, p, None, g["y"].ptr, M, N, -8, ident, e4)),
           ("misaligned x", lambda g: linear(nv, p + 2, p, None, g["y"].ptr, M, N, K, ident, e4)),
           ("misaligned w", lambda g: linear(nv, p, p + 8, None, g["y"].ptr, M, N, K, ident, e4)),
           ("table format without a table, w", lambda g: linear(nv, p, p, None, g["y"].ptr, M, N, K, ident, table_without_table)),
           ("table format without a table, x", lambda g: linear(nv, p, p, None, g["y"].ptr, M, N, K, table_without_table, e4))]

    def b(g, B=1, M=M, N=N, K=K, a=p, bb=p, lda=None, sa=None, ldb_k=1, ldb_n=None, sb=None, qa=ident, qb=e4):
        lda = K if lda is None else lda
        return bmm(nv, a, bb, g["y"].ptr, B, M, N, K, lda, M * lda if sa is None else sa, ldb_k, K if ldb_n is None else ldb_n,
                   N * K if sb is None else sb, qa, qb)

    bm = [("K % 8 != 0", lambda g: b(g, K=12, lda=16, ldb_n=16)),
          ("K == 0", lambda g: b(g, K=0, lda=16, ldb_n=16)),
          ("misaligned a", lambda g: b(g, a=p + 2)),
          ("misaligned b", lambda g: b(g, bb=p + 4)),
          ("table format without a table", lambda g: b(g, qb=table_without_table)),
          ("neither leading dimension of B is 1", lambda g: b(g, ldb_k=16, ldb_n=32)),
          ("B > 65535", lambda g: b(g, B=65536, M=1, N=8, K=8)),
          ("N % 8 != 0 in NN", lambda g: b(g, N=12, ldb_k=16, ldb_n=1)),
          ("lda % 8 != 0", lambda g: b(g, lda=20)),
          ("sb % 8 != 0", lambda g: b(g, B=2, sb=N * K + 4))]
    for name, fn in lin:
        refused(fn, y, "qt_linear_fq_bf16: " + name)
    for name, fn in bm:
        refused(fn, y, "qt_bmm_fq_bf16: " + name)
    assert e4.slot() == 0x12340000


def test_empty_problems_are_ok_and_write_nothing(nv):
    buf = dev(np.zeros(4096, np.uint16))
    p = buf.data_ptr()
    ident, e4 = Operand(nv, PASS), Operand(nv, gc.BMode("e4m3", None, True))
    e4.fill(0x12340000)
    g = Guarded((64,), np.uint16)
    for M, N in ((0, 16), (16, 0), (0, 0)):
        assert linear(nv, p, p, None, g.ptr, M, N, 16, ident, e4) == OK
        assert bmm(nv, p, p, g.ptr, 2, M, N, 16, 16, 256, 1, 16, 256, ident, e4) == OK
    assert bmm(nv, p, p, g.ptr, 0, 16, 16, 16, 16, 256, 1, 16, 256, ident, e4) == OK
    torch.cuda.synchronize()
    assert g.untouched() and e4.slot() == 0x12340000


# ---- Tier 3 -----------------------------------------------------------------------------------------------------------------------------
def assert_products_close(got_bits, ref64, what):
    from test_gpu_parity import _products_close                          # the project's own criterion, as it stands
    ok, share, excess = gc.products_close(got_bits, ref64)
    print(f"\n[gemm_fq] {what}: bit-equal share {share:.5f}, worst excess over the bound {excess:.3e}")
    assert _products_close(torch.from_numpy(got_bits.view(np.int16).copy()).view(torch.bfloat16), torch.from_numpy(ref64)), what
    assert ok, what


@pytest.mark.parametrize("dtype,scale", gc.TOL_MODES)
@pytest.mark.parametrize("shape", gc.TOL_LINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_general_scales(nv, shape, dtype, scale):
    """N(0, 1) activations, N(0, 0.05) weights at calibrated (non-power-of-two) scales: every element within 2^-7 |ref| + 2^-16 max|ref|
    of the fp64 product of the oracle-quantized operands plus bias, at most 1e-2 of them different from that product rounded once.
    Bit-equal shares observed on the MI355X (printed with -s; not known beforehand): 1.00000 for all three modes at K = 136;
    0.99977 (e4m3), 0.99998 (int8), 0.99991 (int4) at K = 1000; 0.99993 for the NN bmm below."""
    M, N, K = shape
    c = gc.tol_operands(shape, sum(shape))
    mode = gc.BMode(dtype, scale, True)
    ref64, _ = gc.exact_product(c["a"], mode.fq(c["w"]), c["bias"])
    x, w, b = dev(c["a"]), dev(c["w"]), dev(c["bias"])
    qx, qw = Operand(nv, PASS), Operand(nv, mode)

    def go(g):
        qw.fill(0)
        return linear(nv, x, w, b, g["y"].ptr, M, N, K, qx, qw)

    what = f"linear {shape} {dtype} at {scale}"
    assert_products_close(launch(go, {"y": ((M, N), np.uint16)}, what)["y"], ref64, what)
    assert qw.slot() == int((c["w"] & 0x7FFF).max()) << 16


def test_bmm_nn_general_scales(nv):
    Bn, M, N, K = gc.TOL_BMM_NN
    c = gc.tol_operands((M, N, K), M + N + K, Bn)
    mode = gc.BMode("e4m3", 0.037, False)
    ref64, _ = gc.exact_product(c["a"], mode.fq(c["w"]))
    a, b = dev(c["a"]), dev(np.ascontiguousarray(np.swapaxes(c["w"], 1, 2)))
    qa, qb = Operand(nv, PASS), Operand(nv, mode)
    y = launch(lambda g: bmm(nv, a, b, g["y"].ptr, Bn, M, N, K, K, M * K, N, 1, K * N, qa, qb), {"y": ((Bn, M, N), np.uint16)}, "bmm NN")["y"]
    assert_products_close(y, ref64, f"bmm NN {gc.TOL_BMM_NN} e4m3 at 0.037")


# ---- non-finite weights -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", gc.NONFINITE_MODES, ids=lambda m: m.id)
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_one_non_finite_weight_stays_in_its_column(nv, mode, bad):
    """One NaN in W: exactly column n of y is NaN.  One +Inf: what the format makes of it (the oracle's fq): a finite value under a
    saturating format, NaN or Inf -- then +-Inf by the sign of x -- otherwise; in that column only, everything else as without it."""
    M, N, K = gc.NONFINITE_SHAPE
    n0, k0 = 37, 21
    c = gc.tol_operands((M, N, K), 5)
    c["w"][n0, k0] = NAN16 if bad == "nan" else 0x7F80
    wq = mode.fq(c["w"])
    with np.errstate(invalid="ignore"):
        ref64, _ = gc.exact_product(c["a"], wq, c["bias"])
    x, w, b = dev(c["a"]), dev(c["w"]), dev(c["bias"])
    qx, qw = Operand(nv, PASS), Operand(nv, mode)

    def go(g):
        qw.fill(0)
        return linear(nv, x, w, b, g["y"].ptr, M, N, K, qx, qw)

    what = f"{bad} in W, {mode.id}"
    got = o.bf16_to_f32(launch(go, {"y": ((M, N), np.uint16)}, what)["y"])
    others = np.ones(N, bool)
    others[n0] = False
    if bad == "nan":
        assert np.isnan(ref64[:, n0]).all()
    assert np.isfinite(ref64[:, others]).all() and np.isfinite(got[:, others]).all(), what
    assert np.array_equal(np.isnan(got[:, n0]), np.isnan(ref64[:, n0])), what
    assert np.array_equal(np.isposinf(got[:, n0]), np.isposinf(ref64[:, n0])) and np.array_equal(np.isneginf(got[:, n0]), np.isneginf(ref64[:, n0])), what
    fin = np.isfinite(ref64)
    ok, share, excess = gc.products_close(o.f32_to_bf16(np.where(fin, got, 0).astype(np.float32)), np.where(fin, ref64, 0.0))
    assert ok, (what, share, excess)
    if mode.obs:
        assert qw.slot() == int((c["w"] & 0x7FFF).max()) << 16                    # NaN and Inf patterns win the integer maximum
