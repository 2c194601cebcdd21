"""Group-wise affine on the device: qt_fake_quant_gwa_*, qt_quantize_blocks_* and qt_dequantize_blocks_* (csrc/qt_groupwise.hip)
through the C ABI, the module and the quantized_ops operators.  Every comparison is bit for bit (NaNs canonicalised, no element left
out): against the numpy oracle for the C ABI, against the package's CPU path and the extracted torch composite above it.

The input recipe (recipe()) puts zero blocks, constant blocks, an all-negative stretch, +Inf, -Inf, NaN and a 3e38 element into
a normal draw with per-row magnitudes 1e-3 .. 1e2, so sf = 0 -> 1, NaN / Inf propagation and an overflowing hi - lo all occur.

Layouts: the tensor is [outer][n][inner]; inner == 1 runs fq_gwa_last_kernel (grid-stride loop, at most kGwaLastBlocksPerCu = 8
blocks of 256 vectors per compute unit; test_c_abi_equals_the_oracle_over_two_grid_trips is sized from that cap), inner > 1 runs
fq_gwa_strided_kernel (one workgroup per tile, no grid loop: no large case)."""
import ctypes
from dataclasses import asdict

import numpy as np
import pytest
import torch

from oracle import qt_oracle as o

pytestmark = pytest.mark.gpu

RANGES = [(0, 15), (-8, 7), (0, 3), (0, 255)]
CASES = [((8, 512), -1, 32), ((8, 512), -1, 128), ((6, 256), -1, 256), ((2, 3, 128, 64), -1, 16), ((2, 3, 128, 64), -2, 64),
         ((4, 256, 40), -2, 64)]
GUARD = 64                                         # poisoned elements on each side of every output of the C ABI launches
LAST_BLOCKS_PER_CU = 8                             # csrc/qt_groupwise.hip kGwaLastBlocksPerCu


def case_id(c):
    return f"{'x'.join(map(str, c[0]))}-ax{c[1]}-bs{c[2]}"


@pytest.fixture(scope="module")
def nv():
    from quantized_training import _native
    assert torch.cuda.is_available(), "these tests need the GPU"
    _native.lib()
    return _native


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def recipe(shape, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 2, shape[:-1] + (1,))).astype(np.float32)
    f = x.reshape(-1)
    f[0:256] = 0.0
    f[256:512] = 1.5
    f[512:768] = -np.abs(f[512:768])
    f[800], f[1100], f[1400] = np.inf, -np.inf, np.nan
    f[-1] = 3.0e38
    return x


class Io:
    def __init__(self, name):
        self.name, self.bf16 = name, name == "bf16"
        self.torch_bits = torch.int16 if self.bf16 else torch.int32
        self.np_signed = np.int16 if self.bf16 else np.int32
        self.np_bits = np.uint16 if self.bf16 else np.uint32
        self.dtype = torch.bfloat16 if self.bf16 else torch.float32
        self.poison = 0x7FA5 if self.bf16 else 0x7FA5A5A5          # a NaN with a payload no kernel produces

    def __repr__(self):
        return self.name

    def bits_of(self, x):
        """float32 array -> (bit patterns, the values those patterns hold as float32)"""
        if self.bf16:
            b = o.f32_to_bf16(x).reshape(x.shape)
            return b, o.bf16_to_f32(b).reshape(x.shape)
        x = np.ascontiguousarray(x, np.float32)
        return x.view(np.uint32), x

    def ref_bits(self, a):
        a = np.ascontiguousarray(a, np.float32)
        return self.canon(o.f32_to_bf16(a).reshape(a.shape) if self.bf16 else a.view(np.uint32))

    def canon(self, b):
        return o.canon_nan16(b) if self.bf16 else o.canon_nan32(b)

    def to_dev(self, bits):
        return torch.from_numpy(np.ascontiguousarray(bits).view(self.np_signed)).cuda()

    def tensor(self, bits, device="cuda"):
        return torch.from_numpy(np.ascontiguousarray(bits).view(self.np_signed)).to(device).view(self.dtype)

    def host(self, t):
        """any tensor of this dtype (or its bit view) -> canonical bit patterns on the host"""
        t = t.detach().contiguous()
        if t.dtype == self.dtype:
            t = t.view(self.torch_bits)
        return self.canon(t.cpu().numpy().view(self.np_bits))

    def guarded(self, numel):
        """A poisoned device buffer with GUARD elements on each side of `numel` payload elements (payload 16-byte aligned)."""
        buf = torch.full((numel + 2 * GUARD,), self.poison, dtype=self.torch_bits, device="cuda")
        return buf, buf[GUARD:GUARD + numel]

    def guards_intact(self, buf):
        raw = buf.cpu().numpy().view(self.np_bits)
        return bool((raw[:GUARD] == self.poison).all() and (raw[-GUARD:] == self.poison).all())


BF16, F32 = Io("bf16"), Io("f32")
IOS = [BF16, F32]


def view_of(shape, ax):
    ax %= len(shape)
    return int(np.prod(shape[:ax], dtype=np.int64)), shape[ax], int(np.prod(shape[ax + 1:], dtype=np.int64))


def launch_gwa(nv, io, xbits, shape, ax, bs, qmin, qmax, scale_lut=None):
    """qt_fake_quant_gwa_* with poisoned, guarded outputs -> canonical (y, scale, zero_point) bits; asserts the guards."""
    outer, n, inner = view_of(shape, ax)
    numel = outer * n * inner
    xd = io.to_dev(xbits.reshape(-1))
    ybuf, y = io.guarded(numel)
    sbuf, s = io.guarded(numel // bs)
    zbuf, z = io.guarded(numel // bs)
    fn = getattr(nv.lib(), "qt_fake_quant_gwa_" + io.name)
    nv.check(fn(xd.data_ptr(), y.data_ptr(), s.data_ptr(), z.data_ptr(), outer, n, inner, bs, float(qmin), float(qmax),
                scale_lut.data_ptr() if scale_lut is not None else None, stream()), "qt_fake_quant_gwa")
    torch.cuda.synchronize()
    for name, buf in (("y", ybuf), ("scale", sbuf), ("zero_point", zbuf)):
        assert io.guards_intact(buf), f"{name}: a guard word was overwritten"
    return io.host(y), io.host(s), io.host(z)


def assert_same(io, got, exp, what):
    exp = exp.reshape(-1)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{what}: {bad.size} of {exp.size} differ, first at {bad[:4]}: got {got[bad[:4]]} expected {exp[bad[:4]]}"


# ---- 1. the C ABI against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io", IOS, ids=repr)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_c_abi_equals_the_oracle(nv, case, io):
    shape, ax, bs = case
    bits, x = io.bits_of(recipe(shape, seed=bs + len(shape)))
    for qmin, qmax in RANGES:
        y, s, z = launch_gwa(nv, io, bits, shape, ax, bs, qmin, qmax)
        ey, es, ez = o.group_wise_affine_fake_quant(x, io.bf16, ax, bs, qmin, qmax)
        assert_same(io, y, io.ref_bits(ey), f"y {qmin, qmax}")
        assert_same(io, s, io.ref_bits(es), f"scale {qmin, qmax}")
        assert_same(io, z, io.ref_bits(ez), f"zero_point {qmin, qmax}")


@pytest.mark.parametrize("qrange", RANGES, ids=str)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_c_abi_equals_the_oracle_over_two_grid_trips(nv, io, qrange):
    """Last-axis layout, 256 vectors more than the grid holds: block 0 takes a second trip, every other block idles through it."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per = 8 if io.bf16 else 4
    cols = 64 * per                                               # 64 vectors per row
    rows = cus * LAST_BLOCKS_PER_CU * 256 // 64 + 4               # grid capacity + 256 vectors
    bits, x = io.bits_of(recipe((rows, cols), seed=7))
    y, s, z = launch_gwa(nv, io, bits, (rows, cols), -1, 64, *qrange)
    ey, es, ez = o.group_wise_affine_fake_quant(x, io.bf16, -1, 64, *qrange)
    assert_same(io, y, io.ref_bits(ey), "y")
    assert_same(io, s, io.ref_bits(es), "scale")
    assert_same(io, z, io.ref_bits(ez), "zero_point")


# ---- 2. with a scale map ---------------------------------------------------------------------------------------------------------------
def expect_with_scale_map(x, bf16, ax, bs, qmin, qmax, smap):
    """The oracle's steps with the scale map applied to sf and zp after both are computed (fake_quantize.py:174-182)."""
    F = np.float32
    rd = o.rbf if bf16 else (lambda a: np.asarray(a, F))
    vm = (lambda v: o.bf16_to_f32(o.vmap_bf16(o.f32_to_bf16(v), smap)).reshape(v.shape)) if bf16 else (lambda v: o.vmap_f32(v, smap))
    blocks, a = o._to_blocks(x, ax, bs)
    with np.errstate(all="ignore"):
        mn, mx = np.min(blocks, axis=a + 1), np.max(blocks, axis=a + 1)
        sf = rd(rd(mx - mn) / F(qmax - qmin))
        sf = np.where(sf > 0.0, sf, F(1.0)).astype(F)
        zp = rd(rd(rd(-mn) / sf) + F(qmin))
        sf, zp = vm(sf).astype(F), vm(zp).astype(F)
        se, ze = o._expand_blocks(sf, a, bs, x.shape[a]), o._expand_blocks(zp, a, bs, x.shape[a])
        q = o._clamp(np.rint(rd(rd(x / se) + ze)), F(qmin), F(qmax))
        y = rd(rd(q - ze) * se)
    return y.astype(F), sf, zp


@pytest.mark.parametrize("io", IOS, ids=repr)
@pytest.mark.parametrize("case", [((8, 512), -1, 32), ((2, 3, 128, 64), -2, 64)], ids=case_id)
def test_c_abi_with_a_scale_map(nv, case, io):
    shape, ax, bs = case
    smap = o.get_quantization_map("fp8_e5m3")
    lut = torch.from_numpy(smap.view(np.int16)).cuda()
    bits, x = io.bits_of(recipe(shape, seed=3))
    for qmin, qmax in [(0, 15), (0, 3)]:
        y, s, z = launch_gwa(nv, io, bits, shape, ax, bs, qmin, qmax, lut)
        ey, es, ez = expect_with_scale_map(x, io.bf16, ax, bs, qmin, qmax, smap)
        assert_same(io, y, io.ref_bits(ey), f"y {qmin, qmax}")
        assert_same(io, s, io.ref_bits(es), f"scale {qmin, qmax}")
        assert_same(io, z, io.ref_bits(ez), f"zero_point {qmin, qmax}")


# ---- 3. the module ------------------------------------------------------------------------------------------------------------------------
def module(spec, device):
    import quantized_training as qt
    return qt.FusedAmaxObsFakeQuantize(**asdict(qt.QuantizationSpec.from_str(spec)), device=device)


@pytest.fixture
def kernel_calls(nv, monkeypatch):
    """Counts the launches of the six group-wise entry points."""
    L = nv.lib()
    calls = {}
    for fam in ("fake_quant_gwa", "quantize_blocks", "dequantize_blocks"):
        for io in ("bf16", "f32"):
            name = f"qt_{fam}_{io}"

            def wrapper(*args, _fn=getattr(L, name), _fam=fam):
                calls[_fam] = calls.get(_fam, 0) + 1
                return _fn(*args)
            monkeypatch.setattr(L, name, wrapper)
    return calls


def run_module(spec, xt, device):
    """(y, scale, zero_point) of a fresh module on `device`, or the exception it raises."""
    m = module(spec, device)
    try:
        y = m(xt.to(device))
    except Exception as e:                                       # noqa: BLE001 -- compared by type below
        return e
    return y, m.scale, m.zero_point


def assert_same_outcome(io, got, exp, what):
    if isinstance(exp, Exception):
        assert type(got) is type(exp), f"{what}: {got!r} where the CPU path raises {exp!r}"
        return
    assert not isinstance(got, Exception), f"{what}: raised {got!r}"
    for name, g, e in zip(("y", "scale", "zero_point"), got, exp):
        assert g.dtype == e.dtype and tuple(g.shape) == tuple(e.shape), f"{what} {name}: {g.dtype} {tuple(g.shape)} / {e.dtype} {tuple(e.shape)}"
        pio = io if g.dtype == io.dtype else F32
        if g.dtype not in (torch.bfloat16, torch.float32):
            g, e = g.float(), e.float()
        assert_same(pio, pio.host(g).reshape(-1), pio.host(e), f"{what} {name}")


MODULE_CASES = [("uint4,qs=group_wise_affine,bs=128,ax=-1", (8, 512)), ("int4,qs=group_wise_affine,bs=32,ax=-1", (8, 512)),
                ("uint2,bs=64,qs=group_wise_affine,ax=-2,scale=fp8_e5m3", (2, 3, 128, 64))]


@pytest.mark.parametrize("io", IOS, ids=repr)
@pytest.mark.parametrize("spec,shape", MODULE_CASES, ids=[c[0].split(",")[0] + "-" + c[0].split("ax=")[1][:2] for c in MODULE_CASES])
def test_module_equals_the_cpu_module_and_the_composite(nv, kernel_calls, spec, shape, io):
    from quantized_training.fake_quantize import group_wise_affine_composite
    bits, _ = io.bits_of(recipe(shape, seed=11))
    xt = io.tensor(bits, "cpu")
    exp = run_module(spec, xt, "cpu")
    assert kernel_calls == {}
    got = run_module(spec, xt, "cuda")
    assert kernel_calls == {"fake_quant_gwa": 1}, "the fused kernel did not run"
    assert_same_outcome(io, got, exp, "kernel vs CPU module")
    m = module(spec, "cuda")
    smap = m.scale_qmap.cuda() if m.scale_qmap is not None else None
    sc, zp = torch.empty(0, device="cuda"), torch.empty(0, device="cuda")
    y = group_wise_affine_composite(xt.cuda(), sc, zp, m.ch_axis, m.block_size, m.quant_min, m.quant_max, smap)
    assert kernel_calls == {"fake_quant_gwa": 1}
    assert_same_outcome(io, (y, sc, zp), exp, "device composite vs CPU module")


DECLINED = [("uint4,qs=group_wise_affine,bs=32,ax=-1", (16, 100), torch.bfloat16, "axis length 100"),
            ("uint4,qs=group_wise_affine,bs=32,ax=-2", (4, 64, 20), torch.bfloat16, "inner = 20"),
            ("uint4,qs=group_wise_affine,bs=(1,32),ax=(0,1)", (8, 512), torch.bfloat16, "tuple block size"),
            ("uint4,qs=group_wise_affine,bs=32,ax=-1", (8, 512), torch.float16, "fp16")]


@pytest.mark.parametrize("spec,shape,dtype,why", DECLINED, ids=[d[3] for d in DECLINED])
def test_module_declines_and_the_composite_answers(nv, kernel_calls, spec, shape, dtype, why):
    xt = torch.from_numpy(recipe(shape, seed=5)).to(dtype)
    exp = run_module(spec, xt, "cpu")
    got = run_module(spec, xt, "cuda")
    assert kernel_calls == {}, f"{why}: the kernel ran"
    io = BF16 if dtype == torch.bfloat16 else F32
    if dtype == torch.float16 and not isinstance(exp, Exception):
        assert got[0].dtype == torch.float16
        got, exp = tuple(t.float() for t in got), tuple(t.float() for t in exp)
    assert_same_outcome(io, got, exp, why)


# ---- 4. non-contiguous input -------------------------------------------------------------------------------------------------------------
def test_transposed_key_layout_gives_the_values_of_the_contiguous_copy(nv, kernel_calls):
    spec = "uint2,bs=64,qs=group_wise_affine,ax=-2,scale=fp8_e5m3"
    bits, _ = BF16.bits_of(recipe((2, 128, 3, 64), seed=13))
    k = BF16.tensor(bits).transpose(1, 2)                        # [B, S, H, D] -> [B, H, S, D] view
    assert not k.is_contiguous()
    got = run_module(spec, k, "cuda")
    exp = run_module(spec, k.contiguous(), "cuda")
    assert kernel_calls == {"fake_quant_gwa": 2}
    assert_same_outcome(BF16, got, exp, "transposed")
    assert_same_outcome(BF16, got, run_module(spec, k.cpu(), "cpu"), "transposed vs CPU")


# ---- 5. quantize / dequantize ops ------------------------------------------------------------------------------------------------------------
def qparams(spec, xt):
    """Block scales and zero points of xt in xt's dtype, from the CPU module."""
    m = module(spec, "cpu")
    m(xt)
    s, z = m.calculate_qparams()
    return m, s.to(xt.dtype), z.to(xt.dtype)


@pytest.mark.parametrize("io", IOS, ids=repr)
@pytest.mark.parametrize("shape,ax,bs", [((8, 512), -1, 32), ((2, 3, 128, 64), -2, 64)], ids=["last", "strided"])
def test_blockwise_quantize_dequantize_ops_equal_the_cpu_ops(nv, kernel_calls, shape, ax, bs, io):
    import quantized_training as qt
    Q, DQ = torch.ops.quantized_ops.quantize, torch.ops.quantized_ops.dequantize
    bits, _ = io.bits_of(recipe(shape, seed=17))
    xt = io.tensor(bits, "cpu")
    m, s, z = qparams(f"uint4,qs=group_wise_affine,bs={bs},ax={ax}", xt)
    axes = [ax]
    qmap, in_map, out_map = (qt.get_quantization_map(d, torch.device("cpu")) for d in ("uint4", "int8", "fp8_e4m3"))
    dev = lambda t: None if t is None else t.cuda()               # noqa: E731
    codes = Q(xt, s, z, axes, bs, qmap)
    got = Q(dev(xt), dev(s), dev(z), axes, bs, dev(qmap))
    assert kernel_calls == {"quantize_blocks": 1}
    assert got.dtype == codes.dtype and got.shape == codes.shape
    assert_same(io, io.host(got).reshape(-1), io.host(codes), "quantize")
    for n, (imap, omap) in enumerate([(None, None), (in_map, None), (None, out_map), (in_map, out_map)]):
        exp = DQ(codes, s, z, axes, bs, imap, omap)
        got = DQ(dev(codes), dev(s), dev(z), axes, bs, dev(imap), dev(omap))
        assert kernel_calls["dequantize_blocks"] == n + 1
        assert got.dtype == exp.dtype and got.shape == exp.shape
        assert_same(io, io.host(got).reshape(-1), io.host(exp), f"dequantize in={imap is not None} out={omap is not None}")
    # zero_point=None keeps its old path (the microscaling route)
    before = dict(kernel_calls)
    exp = DQ(codes, s, None, axes, bs)
    got = DQ(dev(codes), dev(s), None, axes, bs)
    expq = Q(xt, s, None, axes, bs, qmap)
    gotq = Q(dev(xt), dev(s), None, axes, bs, dev(qmap))
    assert kernel_calls == before
    assert_same(io, io.host(got).reshape(-1), io.host(exp), "dequantize without zero point")
    assert_same(io, io.host(gotq).reshape(-1), io.host(expq), "quantize without zero point")


def test_lowering_round_trip_reproduces_the_fake_quantized_weight(nv, kernel_calls):
    """What quantize_pt2e._lower_group_wise_affine stores and the dequantize node it leaves: fq(w) -> quantize -> dequantize = fq(w)."""
    torch.manual_seed(0)
    w = torch.randn(64, 256).bfloat16().cuda()
    fq = module("uint4,qs=group_wise_affine,bs=32,ax=-1", "cuda")
    y = fq(w)
    s, z = fq.calculate_qparams()
    s, z = s.to(w.dtype), z.to(w.dtype)
    codes = torch.ops.quantized_ops.quantize(w, s, z, [-1], 32, fq.qmap)
    back = torch.ops.quantized_ops.dequantize(codes, s, z, (-1,), 32)
    assert kernel_calls == {"fake_quant_gwa": 1, "quantize_blocks": 1, "dequantize_blocks": 1}
    assert_same(BF16, BF16.host(back).reshape(-1), BF16.host(y), "round trip")
    assert float(codes.float().min()) >= 0.0 and float(codes.float().max()) <= 15.0


# ---- 6. stream capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,shape", [MODULE_CASES[0], MODULE_CASES[2]], ids=["last", "strided"])
def test_captured_graph_replays_on_refreshed_input(nv, kernel_calls, spec, shape):
    m = module(spec, "cuda")
    b0, _ = BF16.bits_of(recipe(shape, seed=19))
    b1, _ = BF16.bits_of(recipe(shape, seed=23) * 3.0)
    x0, x1 = BF16.tensor(b0), BF16.tensor(b1)
    xs = x0.clone()
    m(xs)                                                        # warm-up: buffers take their shapes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ys = m(xs)
    xs.copy_(x1)
    g.replay()
    torch.cuda.synchronize()
    got = (ys.clone(), m.scale.clone(), m.zero_point.clone())
    exp = run_module(spec, x1, "cuda")
    assert kernel_calls["fake_quant_gwa"] == 3
    assert_same_outcome(BF16, got, exp, "replay")


# ---- 7. guard regions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io", IOS, ids=repr)
@pytest.mark.parametrize("case", [((6, 256), -1, 64), ((4, 256, 40), -2, 64), ((3, 200, 24), -2, 100)], ids=case_id)
def test_partly_idle_last_workgroup_leaves_the_guards_alone(nv, case, io):
    """Shapes whose last workgroup has idle lanes (and, for 100 rows, idle row groups); launch_gwa asserts the poison around y, scale
    and zero_point, and the payload equals the oracle's, so nothing inside was skipped either."""
    shape, ax, bs = case
    bits, x = io.bits_of(recipe(shape, seed=29))
    y, s, z = launch_gwa(nv, io, bits, shape, ax, bs, 0, 15)
    ey, es, ez = o.group_wise_affine_fake_quant(x, io.bf16, ax, bs, 0, 15)
    assert_same(io, y, io.ref_bits(ey), "y")
    assert_same(io, s, io.ref_bits(es), "scale")
    assert_same(io, z, io.ref_bits(ez), "zero_point")


def test_declines_are_answered_before_any_launch(nv):
    L = nv.lib()
    x, y, s, z = (torch.zeros(4096, dtype=torch.int16, device="cuda") for _ in range(4))
    p = x.data_ptr()
    gwa = lambda *a: L.qt_fake_quant_gwa_bf16(*a, stream())       # noqa: E731
    assert gwa(p, y.data_ptr(), s.data_ptr(), z.data_ptr(), 8, 512, 1, 32, 0.0, 15.0, None) == 0
    assert gwa(None, p, p, p, 8, 512, 1, 32, 0.0, 15.0, None) == nv.QT_ERR_BAD_ARG
    assert gwa(p, p, p, p, 8, 512, 1, 48, 0.0, 15.0, None) == nv.QT_ERR_BAD_ARG
    assert gwa(p, p, p, p, 8, 512, 1, 4, 0.0, 15.0, None) == nv.QT_ERR_BAD_ARG
    assert gwa(p, p, p, p, 8, 64, 8, 1024, 0.0, 15.0, None) == nv.QT_ERR_BAD_ARG
    assert gwa(p, p, p, p, 8, 500, 1, 32, 0.0, 15.0, None) == nv.QT_ERR_UNALIGNED
    assert gwa(p, p, p, p, 8, 64, 4, 32, 0.0, 15.0, None) == nv.QT_ERR_UNALIGNED
    assert gwa(p + 2, p, p, p, 8, 512, 1, 32, 0.0, 15.0, None) == nv.QT_ERR_UNALIGNED
    assert gwa(p, p, p, p, 8, 512, 1, 32, 3.0, 3.0, None) == nv.QT_ERR_BAD_ARG
    assert gwa(None, None, None, None, 0, 512, 1, 32, 0.0, 15.0, None) == 0
    assert L.qt_quantize_blocks_bf16(p, p, p, p, 8, 512, 1, 32, None, stream()) == nv.QT_ERR_BAD_ARG
    assert L.qt_dequantize_blocks_f32(p, p, p, None, 8, 512, 1, 32, None, None, stream()) == nv.QT_ERR_BAD_ARG
    assert L.qt_dequantize_blocks_f32(p, p, p, p, 8, 512, 1, 512, None, None, stream()) == nv.QT_ERR_BAD_ARG
    torch.cuda.synchronize()
