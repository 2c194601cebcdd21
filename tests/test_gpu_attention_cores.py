"""The forward attention cores at every variant, against the interval oracle (oracle.attention_interval).

  qt_attention_fq_bf16 / _live_bf16 / _out_bf16      csrc/qt_attention.hip        two passes, online row sum          family "fq"
  qt_value_t_rows + qt_attention_rows_bf16           csrc/qt_attention_rows.hip   score strip in registers            family "rows"
  qt_value_codes_t + qt_attention_fp8                csrc/qt_attention_fp8.hip    the same on FP8 codes               family "fp8"

The inputs (oracle/attention_cases.py) are small integers times a power of two, so the logits are bit-defined and almost every output
element is decided to the bit; tests/test_oracle_attention_cpu.py asserts, without a GPU, what is relied on here (exact score sums, the
decided shares, the NaN rows).  Every case goes through the C ABI into guarded buffers, twice (bit-identical).  O and the observer's amax
slot must be inside their intervals -- bit equality on the decided elements, NaN exactly where the oracle has NaN -- and the equivalent
launch forms (mask read / row extents / device flag, plain map / row form, observer on / off, the output modes) must agree bit for bit.
A refused call writes nothing.

Run on the MI355X box:  python -m pytest tests/test_gpu_attention_cores.py -m gpu -q -s
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import attention_cases as ac
from oracle import qt_oracle as o

from kernel_launch import GUARD, dev, inside, launch, nv, print_stats, refused, same, stream, table_format  # noqa: F401

pytestmark = pytest.mark.gpu

FQ_NAMES = [c.name for c in ac.fq_cases()]
ROWS_NAMES = [c.name for c in ac.rows_cases()]
FP8_NAMES = [c.name for c in ac.fp8_cases()]


def teardown_module(module):
    print_stats("attention")


@pytest.fixture(scope="module")
def cases():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {(c.family, c.name): c for c in ac.all_cases(cus)}


def _ptr(t):
    return None if t is None else t.data_ptr()


class Inputs:
    """A case's tensors on the device; the mask's row extents come from the device scan and must be the case's own."""

    def __init__(self, nv, c):
        self.c = c
        self.q, self.k, self.v = dev(c.q), dev(c.k), dev(c.v)
        self.mask = None if c.mask is None else dev(c.mask_buffer())
        self.ms = c.mask_strides()
        self.rl = self.irr = None
        self.ls = (0, 0, 0)
        self.irregular = 0
        if c.mask is not None and c.live:
            rows = c.mask_rows()
            buf = torch.full((rows + 1,), -7, dtype=torch.int32, device="cuda")
            nv.check(nv.lib().qt_mask_row_live_checked(self.mask.data_ptr(), rows, c.Sk, c.row_stride, buf.data_ptr(), buf.data_ptr() + 4 * rows, stream()),
                     "qt_mask_row_live_checked")
            ext, self.irregular = c.extents()
            got = buf.cpu().numpy()
            assert np.array_equal(got[:-1], ext) and int(got[-1]) == self.irregular, f"{c.name}: row extents"
            self.buf, self.rl, self.irr, self.ls = buf, buf.data_ptr(), buf.data_ptr() + 4 * rows, c.live_strides()


def _format(nv, c, form=None):
    """(qt_format, device map) of the probabilities' fake-quantizer in the case's form."""
    if (form or c.form) == "rows":
        return table_format(nv, c.fmt)
    return nv.format_for(c.fmt), dev(nv.build_map_u16(c.fmt))


def _bhsd(out):
    """[B, Sq, H, D] as the kernels write it -> [B, H, Sq, D] as the oracle has it."""
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3))


def _check_amax(iv, r, what, family):
    bits = int(r["amax"][0])
    assert bits & 0xFFFF == 0, f"{what}: the amax slot holds a bf16 value"
    inside(iv.amax, np.array([bits >> 16], np.uint16), what + " amax", family + " amax")


# ---- qt_attention_fq_bf16 / _live_bf16 / _out_bf16 ------------------------------------------------------------------------------------------
def _fq_launch(nv, c, x, entry, fmt, lut, what, obs=False, out_fq=0):
    L = nv.lib()
    scale = None if c.scale is None else torch.tensor([c.scale], dtype=torch.float32, device="cuda")
    shape = (c.B, c.Sq, c.H, c.D)
    head = (x.q.data_ptr(), x.k.data_ptr(), x.v.data_ptr(), _ptr(x.mask))
    dims = (c.B, c.H, c.Sq, c.Sk, c.D, *x.ms, c.scaling, ctypes.byref(fmt), lut.data_ptr())

    def fn(g):
        amax = None
        if obs:
            g["amax"].raw[GUARD:GUARD + 4] = 0                     # the slot the observer raises
            amax = g["amax"].ptr
        if entry == "read":
            return L.qt_attention_fq_bf16(*head, g["out"].ptr, *dims, _ptr(scale), amax, stream())
        if entry == "live":
            return L.qt_attention_fq_live_bf16(*head, g["out"].ptr, *dims, _ptr(scale), amax, out_fq, x.rl, *x.ls, x.irr, stream())
        return L.qt_attention_fq_out_bf16(*head, g["out"].ptr, *dims, stream())

    specs = {"out": (shape, np.uint16)}
    if obs:
        specs["amax"] = ((1,), np.uint32)
    return launch(fn, specs, what)


@pytest.mark.parametrize("name", FQ_NAMES)
def test_attention_fq_every_variant(nv, cases, name):
    """The two-pass core: every case inside its interval, and its launch forms bit-identical."""
    c = cases["fq", name]
    x = Inputs(nv, c)
    fmt, lut = _format(nv, c)
    iv = c.intervals()
    what = f"qt_attention_fq_bf16 {name}"
    r = _fq_launch(nv, c, x, "read", fmt, lut, what, obs=c.obs)
    inside(iv.out, _bhsd(r["out"]), what, "attention_fq")
    if c.readout is not None:                                     # V = identity on a window of keys: the output IS P' of those keys
        inside(iv.probs.rows((Ellipsis, slice(c.readout, c.readout + c.D))), _bhsd(r["out"]), what + " P'", "attention_fq P'")
    if c.obs:
        _check_amax(iv, r, what, "attention_fq")
        same(_fq_launch(nv, c, x, "read", fmt, lut, what + " without the observer")["out"], r["out"], what + ": observer on / off")
    if c.form == "rows":                                          # the row table in LDS and the gather from the map: the same function
        pf, pl = _format(nv, c, "plain")
        same(_fq_launch(nv, c, x, "read", pf, pl, what + " plain map")["out"], r["out"], what + ": row form / plain map")
    if c.live:                                                    # the mask's row extents and the device flag in place of the mask scan
        rl = _fq_launch(nv, c, x, "live", fmt, lut, what + " live", obs=c.obs)
        same(rl["out"], r["out"], what + ": live / mask read")
        if c.obs:
            same(rl["amax"], r["amax"], what + ": live / mask read, amax")
    if c.out_fq:                                                  # the consumer's fake-quantizer on the way out
        ivq = c.intervals(out_fq=True)
        ro = _fq_launch(nv, c, x, "out", fmt, lut, what + " out_fq")
        inside(ivq.out, _bhsd(ro["out"]), what + " out_fq", "attention_fq")
        same(ro["out"], o.vmap_bf16(r["out"], c.qmap()), what + ": out_fq is the map of the plain result")
        if c.live:
            same(_fq_launch(nv, c, x, "live", fmt, lut, what + " live out_fq", out_fq=1)["out"], ro["out"], what + ": live out_fq / _out_bf16")


def test_attention_fq_refusals(nv, cases):
    """What the entry points do not take: an error status, nothing written."""
    L = nv.lib()
    c = cases["fq", "sq64_sk60_d64_e5m2_padding"]
    x = Inputs(nv, c)
    fmt, lut = _format(nv, c)
    big = dev(np.zeros(max(c.q.size, c.k.size), np.uint16))
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    spec = {"out": ((c.B, c.Sq, c.H, c.D), np.uint16)}
    ptrs = (big.data_ptr(), big.data_ptr(), big.data_ptr())
    tail = (c.scaling, ctypes.byref(fmt), lut.data_ptr())

    def plain(g, B=c.B, H=c.H, Sq=c.Sq, Sk=c.Sk, D=c.D, mask=None, ms=(0, 0, 0), out_off=0, scale=None):
        return L.qt_attention_fq_bf16(*ptrs, mask, g["out"].ptr + out_off, B, H, Sq, Sk, D, *ms, *tail, scale, None, stream())

    refused(lambda g: plain(g, Sk=ac.FQ_REFUSED_SK), spec, "Sk % 4 != 0")
    refused(lambda g: plain(g, D=ac.FQ_REFUSED_D), spec, "head_dim 32")
    refused(lambda g: plain(g, B=ac.REFUSED_BH, H=1), spec, "B * H > 65535")
    refused(lambda g: plain(g, mask=x.mask.data_ptr(), ms=(0, 0, ac.FQ_REFUSED_MASK_STRIDE)), spec, "a mask stride that is no multiple of 4")
    refused(lambda g: plain(g, out_off=2), spec, "a misaligned out")
    refused(lambda g: L.qt_attention_fq_live_bf16(*ptrs, x.mask.data_ptr(), g["out"].ptr, c.B, c.H, c.Sq, c.Sk, c.D, *x.ms, *tail, one.data_ptr(), None, 1,
                                                  x.rl, *x.ls, x.irr, stream()), spec, "out_fq together with a scale")
    refused(lambda g: L.qt_attention_fq_live_bf16(*ptrs, x.mask.data_ptr(), g["out"].ptr, c.B, c.H, c.Sq, c.Sk, c.D, *x.ms, *tail, None, None, 0,
                                                  x.rl, *x.ls, None, stream()), spec, "row_live without the flag")


# ---- qt_value_t_rows + qt_attention_rows_bf16 -----------------------------------------------------------------------------------------------
def _rows_slot(Sk):
    key = np.arange(Sk)
    return (key & ~31) | (((key >> 2) & 3) << 3) | (((key >> 4) & 1) << 2) | (key & 3)


def _rows_value_pass(nv, c, x, fmt, lut):
    """fq_v(v) transposed to [B, H, D, Sk], the keys of every 32-chunk in the k-slot order of the P.V instruction; checked element for
    element (this is where an off-grid v is quantized)."""
    what = f"qt_value_t_rows {c.name}"
    s = c.Sk * c.D
    r = launch(lambda g: nv.lib().qt_value_t_rows(x.v.data_ptr(), g["vt"].ptr, c.B, c.H, c.Sk, c.D, c.H * s, s, c.D, ctypes.byref(fmt), lut.data_ptr(), stream()),
               {"vt": ((c.B, c.H, c.D, c.Sk), np.uint16)}, what)
    want = np.empty_like(r["vt"])
    want[..., _rows_slot(c.Sk)] = c.vq().transpose(0, 1, 3, 2)
    same(r["vt"], want, what)
    if c.v_offgrid:
        assert (c.vq() != c.v).mean() > 0.5, "the value pass has something to quantize"
    return dev(r["vt"])


@pytest.mark.parametrize("name", ROWS_NAMES)
def test_attention_rows_every_variant(nv, cases, name):
    """The table-format core with the strip in registers: value pass, then every mask form, with and without out_fq."""
    L = nv.lib()
    c = cases["rows", name]
    x = Inputs(nv, c)
    fmt, lut = _format(nv, c)
    vt = _rows_value_pass(nv, c, x, fmt, lut)
    shape = (c.B, c.Sq, c.H, c.D)

    def run(out_fq, live, what):
        rl, ls, irr = (x.rl, x.ls, x.irr) if live else (None, (0, 0, 0), None)
        return launch(lambda g: L.qt_attention_rows_bf16(x.q.data_ptr(), x.k.data_ptr(), vt.data_ptr(), _ptr(x.mask), *x.ms, rl, *ls, irr, g["out"].ptr, out_fq,
                                                         ctypes.byref(fmt), lut.data_ptr(), c.B, c.H, c.Sq, c.Sk, c.D, c.scaling, stream()),
                      {"out": (shape, np.uint16)}, what)["out"]

    what = f"qt_attention_rows_bf16 {name}"
    iv, ivq = c.intervals(), c.intervals(out_fq=True)
    r0 = run(0, False, what)
    inside(iv.out, _bhsd(r0), what, "attention_rows")
    if c.readout is not None:
        inside(iv.probs.rows((Ellipsis, slice(c.readout, c.readout + c.D))), _bhsd(r0), what + " P'", "attention_rows P'")
    r1 = run(1, False, what + " out_fq")
    inside(ivq.out, _bhsd(r1), what + " out_fq", "attention_rows")
    same(r1, o.vmap_bf16(r0, c.qmap()), what + ": out_fq is the map of the plain result")
    if c.live:                                                    # regular masks are then not read at all; irregular ones inside the extents
        same(run(0, True, what + " live"), r0, what + ": row extents / mask read")
        same(run(1, True, what + " live out_fq"), r1, what + ": row extents / mask read, out_fq")


def test_attention_rows_refusals(nv, cases):
    L = nv.lib()
    c = cases["rows", "sq1_sk128_posit8_1_nomask"]
    x = Inputs(nv, c)
    fmt, lut = _format(nv, c)
    plain = nv.format_for(c.fmt)
    big = dev(np.zeros(c.B * c.H * 1152 * c.D, np.uint16))
    spec = {"out": ((c.B, c.Sq, c.H, c.D), np.uint16)}

    def call(g, Sk=c.Sk, f=fmt):
        return L.qt_attention_rows_bf16(x.q.data_ptr(), big.data_ptr(), big.data_ptr(), None, 0, 0, 0, None, 0, 0, 0, None, g["out"].ptr, 0, ctypes.byref(f),
                                        lut.data_ptr(), c.B, c.H, c.Sq, Sk, c.D, c.scaling, stream())

    for Sk in ac.ROWS_REFUSED_SK:
        refused(lambda g: call(g, Sk=Sk), spec, f"Sk = {Sk}")
    refused(lambda g: call(g, f=plain), spec, "a format that is not in row form")
    refused(lambda g: L.qt_value_t_rows(big.data_ptr(), g["out"].ptr, c.B, c.H, c.Sk, c.D, c.H * c.Sk * c.D, c.Sk * c.D, c.D, ctypes.byref(plain), lut.data_ptr(),
                                        stream()), {"out": ((c.B, c.H, c.D, c.Sk), np.uint16)}, "the value pass with a format that is not in row form")


# ---- qt_value_codes_t + qt_attention_fp8 ---------------------------------------------------------------------------------------------------
def _fp8_tables(fmt):
    """(bf16 pattern of every code, NaN canonical): the decode of an FP8 byte."""
    name = "fp8_" + fmt
    vals = o.mx_decode(np.arange(256), name)
    if fmt == "e4m3":
        vals[[0x7F, 0xFF]] = np.nan
    else:
        vals[[0x7C, 0xFC]] = [np.inf, -np.inf]
        vals[[0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF]] = np.nan
    return o.f32_to_bf16(vals.astype(np.float32))


def _fp8_codes(bits, fmt):
    return o.mx_encode(o.bf16_to_f32(bits).astype(np.float64), "fp8_" + fmt).astype(np.uint8)


def _fp8_value_pass(nv, c, x, fmt):
    what = f"qt_value_codes_t {c.name}"
    s = c.Sk * c.D
    r = launch(lambda g: nv.lib().qt_value_codes_t(x.v.data_ptr(), g["vt8"].ptr, c.B, c.H, c.Sk, c.D, c.H * s, s, c.D, ctypes.byref(fmt), stream()),
               {"vt8": ((c.B, c.H, c.D, c.Sk), np.uint8)}, what)
    pos = np.arange(128)
    key_of = (pos & 64) | (((pos >> 2) & 3) << 4) | (((pos >> 4) & 3) << 2) | (pos & 3)        # position p of a 128-block holds key key_of[p]
    codes = _fp8_codes(c.vq(), c.fmt).reshape(c.B, c.H, c.Sk // 128, 128, c.D)[:, :, :, key_of, :]
    same(r["vt8"], codes.transpose(0, 1, 4, 2, 3).reshape(c.B, c.H, c.D, c.Sk), what)
    if c.v_offgrid:
        assert (c.vq() != c.v)[c.v != 0].mean() > 0.5, "the value pass has something to quantize"
    return dev(r["vt8"])


@pytest.mark.parametrize("fmt_name,D", [("e4m3", 64), ("e5m2", 128)])
def test_value_codes_t_quantizes_a_dense_v(nv, fmt_name, D):
    """The FP8 core's value pass on a dense off-grid v (the attention cases hold one key per column): every code, two key blocks."""
    q, k, v, _ = ac._qkv(f"dense_v_{fmt_name}", 1, 2, 1, 256, D, v_offgrid=True)
    c = ac.Case(f"dense_v_{fmt_name}_d{D}", "fp8", q, k, v, fmt=fmt_name, v_offgrid=True)
    x = Inputs(nv, c)
    assert (c.vq() != c.v).mean() > 0.5
    _fp8_value_pass(nv, c, x, nv.format_for(fmt_name))


@pytest.mark.parametrize("name", FP8_NAMES)
def test_attention_fp8_every_variant(nv, cases, name):
    """The FP8 core: the mask forms (read, row extents with the caller's or the device's verdict) and the three output modes.
    Its P'.V runs on the scaled matrix instruction, whose sum of several products spanning many binades is not exact and has no
    documented bound (with dense v and exact-in-fp32 sums, 57 of 16 640 outputs were one bf16 step off the exact sum's rounding at
    e5m2, 256 keys, head_dim 64, and 4 of 33 280 at e4m3, head_dim 128), so these cases hold ONE key per column of v
    (oracle/attention_cases.py): every output is one exact product P'[key] x v, compared to the bit wherever P' is decided."""
    L = nv.lib()
    c = cases["fp8", name]
    x = Inputs(nv, c)
    fmt = nv.format_for(c.fmt)
    fcode = 0 if c.fmt == "e4m3" else 1
    q8, k8 = dev(_fp8_codes(c.q, c.fmt)), dev(_fp8_codes(c.k, c.fmt))
    vt8 = _fp8_value_pass(nv, c, x, fmt)
    shape = (c.B, c.Sq, c.H, c.D)
    decode = _fp8_tables(c.fmt)

    def run(mode, live, what, simple=0, flag=False):
        rl, ls = (x.rl, x.ls) if live else (None, (0, 0, 0))
        specs = {}
        if mode in ("out", "both"):
            specs["out"] = (shape, np.uint16)
        if mode in ("both", "codes"):
            specs["out8"] = (shape, np.uint8)
        return launch(lambda g: L.qt_attention_fp8(q8.data_ptr(), k8.data_ptr(), vt8.data_ptr(), fcode, _ptr(x.mask), *x.ms, rl, *ls, simple, x.irr if flag else None,
                                                   g["out"].ptr if "out" in g else None, g["out8"].ptr if "out8" in g else None,
                                                   ctypes.byref(fmt) if "out8" in g else None, c.B, c.H, c.Sq, c.Sk, c.D, c.scaling, stream()), specs, what)

    what = f"qt_attention_fp8 {name}"
    iv, ivq = c.intervals(), c.intervals(out_fq=True)
    r0 = run("out", False, what)
    inside(iv.out, _bhsd(r0["out"]), what, "attention_fp8")
    if c.readout is not None:
        inside(iv.probs.rows((Ellipsis, slice(c.readout, c.readout + c.D))), _bhsd(r0["out"]), what + " P'", "attention_fp8 P'")
    # out and out8: fq(result) and its codes; codes only: the same codes, and they decode to a value inside the interval
    rb = run("both", False, what + " out + out8")
    inside(ivq.out, _bhsd(rb["out"]), what + " out + out8", "attention_fp8")
    same(rb["out"], o.vmap_bf16(r0["out"], c.qmap()), what + ": out is the map of the plain result")
    same(decode[rb["out8"]], rb["out"], what + ": the codes decode to out")
    rc = run("codes", False, what + " codes only")
    same(rc["out8"], rb["out8"], what + ": codes only / out + out8")
    inside(ivq.out, _bhsd(decode[rc["out8"]]), what + " codes only", "attention_fp8")
    if c.live:
        forms = [("row extents", dict(simple=0)), ("device flag", dict(flag=True))]
        if not x.irregular:
            forms.append(("mask_is_simple", dict(simple=1)))
        for tag, kw in forms:
            same(run("out", True, f"{what} {tag}", **kw)["out"], r0["out"], f"{what}: {tag} / mask read")
        same(run("codes", True, what + " device flag, codes only", flag=True)["out8"], rb["out8"], what + ": device flag, codes only")
