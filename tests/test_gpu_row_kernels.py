"""The row-reduction kernels at every row-length instantiation, against the fp64 restatements of oracle/qt_oracle.py.

Five kernel families pick a template instantiation from the row length (RMSNorm and LayerNorm with their variants, the score softmax
forward and backward, the training LayerNorm, the causal-LM loss).  Each is launched through the C ABI on both sides of every dispatch
boundary, at its shortest row, at the longest the ABI takes and once past it (an error, nothing written).  The data regimes are the ROWS
of one small tensor per case (oracle/row_cases.py), so one launch covers them all.

Everywhere: got in [lo, hi] of the oracle's interval in bf16 value order (bit equality where lo == hi), NaN exactly where the oracle has
NaN, guard bands of a sentinel pattern around every output buffer untouched, a second launch bit-identical to the first.  What the oracle
alone guarantees for these cases (>= 95 % of the well-conditioned elements decided, the closed forms of the degenerate rows) is asserted
without a GPU in tests/test_oracle_rows_cpu.py.

Run on the MI355X box:  python -m pytest tests/test_gpu_row_kernels.py -m gpu -q
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import qt_oracle as o
from oracle import row_cases as rc

from kernel_launch import (GUARD, STATS, Guarded, dev, fq8_single, fq_single, inside, launch, nv, print_stats, refused, same,  # noqa: F401
                           stream, table_format)

pytestmark = pytest.mark.gpu


def teardown_module(module):
    print_stats("rows")


def consumer_args(nv, y8s, dtypes):
    fmts = [nv.format_for(d) for d in dtypes]
    a8 = (ctypes.c_void_p * len(y8s))(*[g.ptr for g in y8s])
    af = (ctypes.POINTER(nv.QtFormat) * len(fmts))(*[ctypes.pointer(f) for f in fmts])
    return a8, af, fmts


# ---- RMSNorm ----------------------------------------------------------------------------------------------------------------------------
RMS_EPS = 1e-6


def rms_plain(nv, x_bits, w_bits, what):
    x, w = dev(x_bits), dev(w_bits)
    rows, cols = x_bits.shape
    return launch(lambda g: nv.lib().qt_rmsnorm_bf16(x.data_ptr(), w.data_ptr(), g["y"].ptr, rows, cols, RMS_EPS, stream()),
                  {"y": ((rows, cols), np.uint16)}, what)["y"]


@pytest.mark.parametrize("cols", rc.RMS_COLS)
def test_rmsnorm_every_row_length(nv, cols):
    """qt_rmsnorm_bf16 against oracle.rmsnorm: NV 2 | 4 | 8 on both sides of 4096 | 4104 and 8192 | 8200, 8 and 16 384 columns; all the
    regimes at once, then 3 rows and 1 row."""
    c = rc.norm_case("rms", cols)
    iv, _ = o.rmsnorm(c["x"], c["w"], RMS_EPS)
    for n in (len(c["names"]),) + rc.RMS_ROW_COUNTS:
        inside(iv.rows(slice(0, n)), rms_plain(nv, c["x"][:n], c["w"], f"rmsnorm {n}x{cols}"), f"rmsnorm {n}x{cols}", "rmsnorm")


def test_rmsnorm_refuses_a_row_past_the_longest(nv):
    cols = rc.RMS_REFUSED_COLS
    x, w = dev(np.zeros((2, cols), np.uint16)), dev(np.zeros(cols, np.uint16))
    refused(lambda g: nv.lib().qt_rmsnorm_bf16(x.data_ptr(), w.data_ptr(), g["y"].ptr, 2, cols, RMS_EPS, stream()), {"y": ((2, cols), np.uint16)},
            "qt_rmsnorm_bf16 at 16392 columns")


@pytest.mark.parametrize("cols", rc.RMS_VARIANT_COLS)
def test_rmsnorm_variants_equal_the_plain_kernel(nv, cols):
    """Every FP8, residual-add, consumers and table variant at NV 2, 4 and 8: y bit-identical to qt_rmsnorm_bf16 on the same input (for
    the residual variants the bf16 sum, which is the oracle's), codes / quantized values those of the single pass on that y."""
    L = nv.lib()
    c = rc.norm_case("rms", cols, residual=True)
    rows = len(c["names"])
    shape = (rows, cols)
    x, res, w = dev(c["x"]), dev(c["res"]), dev(c["w"])
    sum_bits = o.bf16_add(c["x"], c["res"])
    y_x, y_s = rms_plain(nv, c["x"], c["w"], "plain(x)"), rms_plain(nv, sum_bits, c["w"], "plain(sum)")
    inside(o.rmsnorm(c["x"], c["w"], RMS_EPS, c["res"])[0], y_s, f"rmsnorm of the sum, {cols}", "rmsnorm")
    single = {d: (fq8_single(nv, y_x, d), fq8_single(nv, y_s, d)) for d in ("e4m3", "e5m2")}
    fin_x, fin_s = o.canon_nan16(y_x) != 0x7FC0, o.canon_nan16(y_s) != 0x7FC0
    for d in ("e4m3", "e5m2"):
        fmt = nv.format_for(d)
        for with_y in (True, False):
            what = f"qt_rmsnorm_fq8_bf16 {d} {cols} y={with_y}"
            specs = {"y8": (shape, np.uint8)}
            if with_y:
                specs["y"] = (shape, np.uint16)
            r = launch(lambda g: L.qt_rmsnorm_fq8_bf16(x.data_ptr(), w.data_ptr(), g["y"].ptr if with_y else None, g["y8"].ptr, rows, cols, RMS_EPS,
                                                      ctypes.byref(fmt), stream()), specs, what)
            same(r["y8"], single[d][0][1], what, fin_x)
            if with_y:                                            # (this variant writes the quantized values: the plain y through the single pass)
                same(r["y"], single[d][0][0], what)
        # residual add, plain and with one consumer's FP8 output
        what = f"qt_add_rmsnorm_bf16 {d} {cols}"
        r = launch(lambda g: L.qt_add_rmsnorm_bf16(x.data_ptr(), res.data_ptr(), w.data_ptr(), g["sum"].ptr, g["y"].ptr, g["y8"].ptr, rows, cols, RMS_EPS,
                                                  ctypes.byref(fmt), stream()), {"sum": (shape, np.uint16), "y": (shape, np.uint16), "y8": (shape, np.uint8)}, what)
        same(r["sum"], sum_bits, what + " sum")
        same(r["y"], single[d][1][0], what)
        same(r["y8"], single[d][1][1], what, fin_s)
        # ... and the sum written through its own fake-quantizer
        sfmt = nv.format_for("e5m2" if d == "e4m3" else "e4m3")
        what = f"qt_add_rmsnorm_sumfq_bf16 {d} {cols}"
        r = launch(lambda g: L.qt_add_rmsnorm_sumfq_bf16(x.data_ptr(), res.data_ptr(), w.data_ptr(), g["sum"].ptr, g["y"].ptr, g["y8"].ptr, rows, cols,
                                                        RMS_EPS, ctypes.byref(fmt), ctypes.byref(sfmt), stream()),
                   {"sum": (shape, np.uint16), "y": (shape, np.uint16), "y8": (shape, np.uint8)}, what)
        same(r["sum"], fq8_single(nv, sum_bits, "e5m2" if d == "e4m3" else "e4m3")[0], what + " sum")
        same(r["y"], single[d][1][0], what)
        same(r["y8"], single[d][1][1], what, fin_s)
    what = f"qt_add_rmsnorm_bf16 without a format, {cols}"
    r = launch(lambda g: L.qt_add_rmsnorm_bf16(x.data_ptr(), res.data_ptr(), w.data_ptr(), g["sum"].ptr, g["y"].ptr, None, rows, cols, RMS_EPS, None, stream()),
               {"sum": (shape, np.uint16), "y": (shape, np.uint16)}, what)
    same(r["sum"], sum_bits, what + " sum")
    same(r["y"], y_s, what)
    # all consumers in one launch
    for n in (2, 3):
        dts = ("e4m3", "e5m2", "e4m3")[:n]
        for with_res in (False, True):
            what = f"qt_rmsnorm_consumers_bf16 {n} consumers, residual={with_res}, {cols}"
            specs = {"y": (shape, np.uint16), **{f"y8_{i}": (shape, np.uint8) for i in range(n)}}
            if with_res:
                specs["sum"] = (shape, np.uint16)

            def run(g):
                a8, af, _keep = consumer_args(nv, [g[f"y8_{i}"] for i in range(n)], dts)
                return L.qt_rmsnorm_consumers_bf16(x.data_ptr(), res.data_ptr() if with_res else None, w.data_ptr(), g["sum"].ptr if with_res else None,
                                                   g["y"].ptr, rows, cols, RMS_EPS, n, ctypes.cast(a8, ctypes.c_void_p), ctypes.cast(af, ctypes.c_void_p), stream())
            r = launch(run, specs, what)
            k = 1 if with_res else 0
            if with_res:
                same(r["sum"], sum_bits, what + " sum")
            same(r["y"], single[dts[0]][k][0], what)              # y carries the first consumer's quantized values
            for i in range(n):
                same(r[f"y8_{i}"], single[dts[i]][k][1], what + f" codes {i}", fin_s if with_res else fin_x)
    # one row-form table format
    fmt, lut = table_format(nv, "posit8_1")
    assert fmt.kind == nv.QT_FMT_LUT and fmt.p1 & 1, "the table format did not come back in its row form"
    for with_res in (False, True):
        what = f"qt_rmsnorm_map_bf16 residual={with_res}, {cols}"
        specs = {"y": (shape, np.uint16)}
        if with_res:
            specs["sum"] = (shape, np.uint16)
        r = launch(lambda g: L.qt_rmsnorm_map_bf16(x.data_ptr(), res.data_ptr() if with_res else None, w.data_ptr(), g["sum"].ptr if with_res else None,
                                                  g["y"].ptr, rows, cols, RMS_EPS, ctypes.byref(fmt), lut.data_ptr(), 0, stream()), specs, what)
        if with_res:
            same(r["sum"], sum_bits, what + " sum")
        same(r["y"], fq_single(nv, y_s if with_res else y_x, fmt, lut), what)


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------
def ln_launch(nv, c, n, eps, what, dtype=None, yq=True):
    x, w, b = dev(c["x"][:n]), dev(c["w"]), dev(c["b"])
    res = dev(c["res"][:n]) if c["res"] is not None else None
    cols = c["x"].shape[1]
    specs = {"y": ((n, cols), np.uint16)}
    fmt = None
    if dtype is not None:
        fmt = nv.format_for(dtype)
        specs["y8"] = ((n, cols), np.uint8)
        if yq:
            specs["yq"] = ((n, cols), np.uint16)
    return launch(lambda g: nv.lib().qt_layernorm_bf16(x.data_ptr(), res.data_ptr() if res is not None else None, w.data_ptr(), b.data_ptr(), g["y"].ptr,
                                                       g["yq"].ptr if "yq" in g else None, g["y8"].ptr if "y8" in g else None, n, cols, eps,
                                                       ctypes.byref(fmt) if fmt is not None else None, stream()), specs, what)


@pytest.mark.parametrize("cols", rc.LN_COLS + rc.LN_CONST_COLS)
def test_layernorm_every_row_length(nv, cols):
    """qt_layernorm_bf16 against oracle.layernorm: the one-wave kernel with one vector, with the upper lanes' second vector absent and
    full (8, 512 | 520, 1024), the workgroup kernel at NV 2 | 4 | 8 (1032, 4096 | 4104, 8192 | 8200, 16 384), with and without the residual,
    eps 1e-12 and 1e-5.  A constant row whose sum is exact gives y == bias bit for bit, as torch's does -- at 56, 120 and 1000 columns
    too, where sum * (1 / cols) is not the constant."""
    for residual in (False, True):
        c = rc.norm_case("ln", cols, residual)
        total = len(c["names"])
        for eps in rc.LN_EPS:
            res = o.layernorm(c["x"], c["w"], c["b"], eps, c["res"])
            for n in (total,) + (rc.LN_ROW_COUNTS if cols <= 1024 else (1,)):
                what = f"layernorm {n}x{cols} residual={residual} eps={eps}"
                y = ln_launch(nv, c, n, eps, what)["y"]
                inside(res.y.rows(slice(0, n)), y, what, "layernorm")
                for i, nm in enumerate(c["names"][:n]):
                    if nm.startswith("const") or nm in ("zero", "overflow"):
                        same(y[i], c["b"], what + f": row {nm} must be the bias")


@pytest.mark.parametrize("cols", rc.LN_VARIANT_COLS)
def test_layernorm_variants_equal_the_plain_kernel(nv, cols):
    """The FP8 and consumers variants at the one-wave kernel and at NV 4 and 8 of the workgroup kernel: y bit-identical to the plain
    launch, yq / y8 the single pass on that y."""
    L = nv.lib()
    for residual in (False, True):
        c = rc.norm_case("ln", cols, residual)
        rows = len(c["names"])
        shape = (rows, cols)
        y0 = ln_launch(nv, c, rows, 1e-5, "plain")["y"]
        fin = o.canon_nan16(y0) != 0x7FC0
        single = {d: fq8_single(nv, y0, d) for d in ("e4m3", "e5m2")}
        for d in ("e4m3", "e5m2"):
            for yq in (True, False):
                what = f"qt_layernorm_bf16 {d} yq={yq} {cols} residual={residual}"
                r = ln_launch(nv, c, rows, 1e-5, what, d, yq)
                same(r["y"], y0, what)
                same(r["y8"], single[d][1], what, fin)
                if yq:
                    same(r["yq"], single[d][0], what)
        x, w, b = dev(c["x"]), dev(c["w"]), dev(c["b"])
        res = dev(c["res"]) if residual else None
        for n in (2, 3):
            dts = ("e5m2", "e4m3", "e5m2")[:n]
            what = f"qt_layernorm_consumers_bf16 {n} consumers {cols} residual={residual}"
            specs = {"y": (shape, np.uint16), "yq": (shape, np.uint16), **{f"y8_{i}": (shape, np.uint8) for i in range(n)}}

            def run(g):
                a8, af, _keep = consumer_args(nv, [g[f"y8_{i}"] for i in range(n)], dts)
                return L.qt_layernorm_consumers_bf16(x.data_ptr(), res.data_ptr() if residual else None, w.data_ptr(), b.data_ptr(), g["y"].ptr, g["yq"].ptr,
                                                     rows, cols, 1e-5, n, ctypes.cast(a8, ctypes.c_void_p), ctypes.cast(af, ctypes.c_void_p), stream())
            r = launch(run, specs, what)
            same(r["y"], y0, what)
            same(r["yq"], single[dts[0]][0], what)
            for i in range(n):
                same(r[f"y8_{i}"], single[dts[i]][1], what + f" codes {i}", fin)


# ---- training LayerNorm -----------------------------------------------------------------------------------------------------------------
class Stages:
    """A qt_chain_stage array whose outputs and amax slots sit in guarded buffers; check(): every stage equals its own qt_fake_quant_bf16
    launch on the tensor it reads, amax included (the logic of tests/test_gpu_parity.py::_chain_setup)."""

    def __init__(self, nv, dtype, scales, src, shape):
        self.nv, self.n, self.src, self.shape = nv, len(scales), src, shape
        self.fmt, self.lut = table_format(nv, dtype)
        self.scales = [torch.tensor([s], dtype=torch.float32, device="cuda") for s in scales]

    def specs(self):
        return {**{f"stage{i}": (self.shape, np.uint16) for i in range(self.n)}, **{f"amax{i}": ((1,), np.uint32) for i in range(self.n)}}

    def array(self, g, zero=True):
        arr = (self.nv.QtChainStage * self.n)()
        for i in range(self.n):
            if zero:
                g[f"amax{i}"].raw[GUARD:GUARD + 4] = 0
            arr[i].scale_f32_dev, arr[i].amax_bits_dev, arr[i].out_dev, arr[i].src = self.scales[i].data_ptr(), g[f"amax{i}"].ptr, g[f"stage{i}"].ptr, self.src[i]
        return arr

    def check(self, r, produced, what):
        L = self.nv.lib()
        for i in range(self.n):
            inp = dev(produced if self.src[i] < 0 else r[f"stage{self.src[i]}"])
            want, am = torch.empty_like(inp), torch.zeros(1, dtype=torch.int32, device="cuda")
            self.nv.check(L.qt_fake_quant_bf16(inp.data_ptr(), want.data_ptr(), inp.numel(), ctypes.byref(self.fmt), self.lut.data_ptr(), self.scales[i].data_ptr(),
                                               am.data_ptr(), stream()), "qt_fake_quant_bf16")
            torch.cuda.synchronize()
            assert np.array_equal(r[f"stage{i}"], want.cpu().numpy().view(np.uint16)), f"{what}: stage {i}"
            assert int(r[f"amax{i}"][0]) == int(am.cpu().numpy().view(np.uint32)[0]), f"{what}: amax of stage {i}"


@pytest.mark.parametrize("cols", rc.TRAIN_COLS)
@pytest.mark.parametrize("rows", rc.TRAIN_ROWS)
def test_layernorm_train_every_row_length(nv, rows, cols):
    """qt_layernorm_train_bf16 / _backward_bf16: y against oracle.layernorm, mean / rstd within their radii, the residual form's sum, the
    stages bit-equal to their own launches; dx in the interval of oracle.layernorm_backward on the kernel's own statistics, dgamma /
    dbeta within d u sum|terms| and one bf16 rounding of the fp64 sums.  257 rows: the reduce launch adds 33 partials (an unrolled trip
    of eight and a tail per wave)."""
    L = nv.lib()
    shape = (rows, cols)
    stats = None
    for residual in (False, True):
        c = rc.train_case(rows, cols, residual)
        x, w, b = dev(c["x"]), dev(c["w"]), dev(c["b"])
        res = dev(c["res"]) if residual else None
        st = Stages(nv, "int8", (0.031, 0.029, 0.04), (-1, -1, -1), shape)
        specs = {"y": (shape, np.uint16), "mean": ((rows,), np.float32), "rstd": ((rows,), np.float32), **st.specs()}
        if residual:
            specs["sum"] = (shape, np.uint16)
        what = f"qt_layernorm_train_bf16 {rows}x{cols} residual={residual}"
        r = launch(lambda g: L.qt_layernorm_train_bf16(x.data_ptr(), w.data_ptr(), b.data_ptr(), g["y"].ptr, g["mean"].ptr, g["rstd"].ptr, rows, cols, 1e-5,
                                                      st.array(g), 3, ctypes.byref(st.fmt), st.lut.data_ptr(), res.data_ptr() if residual else None,
                                                      g["sum"].ptr if residual else None, stream()), specs, what)
        ref = o.layernorm(c["x"], c["w"], c["b"], 1e-5, c["res"])
        inside(ref.y, r["y"], what, "layernorm_train")
        if residual:
            same(r["sum"], ref.sum_bits, what + " sum")
        mean, rstd = r["mean"].astype(np.float64), r["rstd"].astype(np.float64)
        assert np.all(np.abs(mean - ref.mean) <= ref.rho_mean), what + ": mean outside its radius"
        assert np.all((rstd >= ref.rstd_lo) & (rstd <= ref.rstd_hi)), what + ": rstd outside its radius"
        for i, nm in enumerate(c["names"]):
            if nm.startswith("const") or nm in ("zero", "overflow"):
                same(r["y"][i], c["b"], what + f": row {nm} must be the bias")
        st.check(r, r["y"], what)
        if not residual:
            stats = (c, r["mean"], r["rstd"])
    # backward, on the kernel's own statistics
    c, mean_h, rstd_h = stats
    dy, x, w, mean, rstd = dev(c["dy"]), dev(c["x"]), dev(c["w"]), dev(mean_h), dev(rstd_h)
    groups = L.qt_layernorm_train_backward_groups(rows)
    assert groups == (rows + 7) // 8
    for nstage, scales, src in ((1, (2.1e-6,), (-1,)), (2, (2.1e-6, 1.7e-6), (-1, 0))):
        st = Stages(nv, "fp8_e5m2", scales, src, shape)
        specs = {"dx": (shape, np.uint16), "dgamma": ((cols,), np.uint16), "dbeta": ((cols,), np.uint16), "part": ((groups, 3, cols), np.float32), **st.specs()}
        what = f"qt_layernorm_train_backward_bf16 {rows}x{cols}, {nstage} stage(s)"
        r = launch(lambda g: L.qt_layernorm_train_backward_bf16(dy.data_ptr(), x.data_ptr(), w.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g["dx"].ptr, rows, cols,
                                                               st.array(g), nstage, ctypes.byref(st.fmt), st.lut.data_ptr(), -1, g["part"].ptr,
                                                               groups * 3 * cols * 4, g["dgamma"].ptr, g["dbeta"].ptr, None, None, 0, stream()), specs, what)
        dx, dgamma, dbeta = o.layernorm_backward(c["dy"], c["x"], c["w"], mean_h, rstd_h)
        inside(dx, r["dx"], what + " dx", "layernorm_train_backward")
        inside(dgamma, r["dgamma"], what + " dgamma", "layernorm_train_backward dgamma/dbeta")
        inside(dbeta, r["dbeta"], what + " dbeta", "layernorm_train_backward dgamma/dbeta")
        st.check(r, r["dx"], what)


def test_layernorm_train_refuses_a_row_past_the_longest(nv):
    L = nv.lib()
    rows, cols = 2, rc.TRAIN_REFUSED_COLS
    z = dev(np.zeros((rows, cols), np.uint16))
    st = Stages(nv, "int8", (0.03,), (-1,), (rows, cols))
    refused(lambda g: L.qt_layernorm_train_bf16(z.data_ptr(), z.data_ptr(), z.data_ptr(), g["y"].ptr, g["mean"].ptr, g["rstd"].ptr, rows, cols, 1e-5,
                                               st.array(g, zero=False), 1, ctypes.byref(st.fmt), st.lut.data_ptr(), None, None, stream()),
            {"y": ((rows, cols), np.uint16), "mean": ((rows,), np.float32), "rstd": ((rows,), np.float32), **st.specs()},
            "qt_layernorm_train_bf16 at 1032 columns")


# ---- softmax forward --------------------------------------------------------------------------------------------------------------------
SOFTMAX_DTYPES = (None, "e4m3", "e5m2", "int8", "posit8_1")
F8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def softmax_formats(nv):
    out = {}
    for d in SOFTMAX_DTYPES:
        fmt, lut = table_format(nv, d) if d is not None else (nv.format_for(None), None)
        out[d] = (fmt, lut, nv.build_map_u16(d))
    return out


def lp(lut):
    return lut.data_ptr() if lut is not None else None


@pytest.mark.parametrize("cols", rc.SOFTMAX_COLS)
def test_softmax_forward_every_row_length(nv, cols):
    """qt_softmax_fq_probs_bf16 / _bf16 / _fp8: the probabilities in the oracle's interval at 16, 32 and 64 lanes per row and 1, 2, 4 and 8
    vectors per lane (128 | 136, 256 | 264, 512 | 520, 1024 | 1032, 2048 | 2056, 4096), two scalings, no mask / a per-(b, q) mask / a
    per-b padding mask with B = 2; for every format the quantized output is the value map of the kernel's own probabilities, FP8 codes
    decode to it, amax is the kernel's own maximum."""
    L = nv.lib()
    formats = softmax_formats(nv)
    _, counts = rc.softmax_rows_per_group(cols)
    for scaling in rc.SOFTMAX_SCALINGS:
        for mask_kind in rc.SOFTMAX_MASKS:
            c = rc.softmax_case(cols, scaling, mask_kind)
            B, H, Q = c["B"], c["H"], c["Q"]
            shape = (B, H, Q, cols)
            sc = dev(c["scores"])
            mask = dev(c["mask"]) if c["mask"] is not None else None
            mp = mask.data_ptr() if mask is not None else None
            sb, sh, sq = c["strides"]
            iv = o.softmax_interval(c["scores"], np.broadcast_to(c["mask"], shape) if c["mask"] is not None else None, scaling)
            own = None
            for d in SOFTMAX_DTYPES:
                fmt, lut, hmap = formats[d]
                what = f"qt_softmax_fq_probs_bf16 {cols} scaling={scaling} mask={mask_kind} {d}"

                def run(g, fmt=fmt, lut=lut):
                    g["amax"].raw[GUARD:GUARD + 4] = 0
                    return L.qt_softmax_fq_probs_bf16(sc.data_ptr(), mp, g["out"].ptr, g["probs"].ptr, B, H, Q, cols, sb, sh, sq, scaling, ctypes.byref(fmt),
                                                      lp(lut), None, g["amax"].ptr, stream())
                r = launch(run, {"out": (shape, np.uint16), "probs": (shape, np.uint16), "amax": ((1,), np.uint32)}, what)
                if own is None:
                    own = r["probs"]
                    inside(iv, own, what, "softmax")
                assert np.array_equal(r["probs"], own), what + ": the probabilities depend on the format"
                quant = o.canon_nan16(hmap[o.canon_nan16(own)])
                same(r["out"], quant, what + ": out is not the value map of the kernel's own probabilities")
                assert int(r["amax"][0]) == int((own.astype(np.uint32) & 0x7FFF).max()) << 16, what + ": amax"
                plain = launch(lambda g, fmt=fmt, lut=lut: L.qt_softmax_fq_bf16(sc.data_ptr(), mp, g["out"].ptr, B, H, Q, cols, sb, sh, sq, scaling, ctypes.byref(fmt),
                                                                              lp(lut), None, None, stream()), {"out": (shape, np.uint16)}, what + " (no probs)")
                same(plain["out"], r["out"], what + ": qt_softmax_fq_bf16 differs")
                if d in F8:
                    for with_out in (True, False):
                        specs = {"out8": (shape, np.uint8)}
                        if with_out:
                            specs["out"] = (shape, np.uint16)
                        r8 = launch(lambda g: L.qt_softmax_fq_bf16_fp8(sc.data_ptr(), mp, g["out"].ptr if with_out else None, g["out8"].ptr, B, H, Q, cols, sb, sh, sq,
                                                                      scaling, ctypes.byref(fmt), stream()), specs, what + " fp8")
                        if with_out:
                            same(r8["out"], quant, what + ": fp8 variant's values")
                        dec = torch.from_numpy(r8["out8"].copy()).view(F8[d]).float().bfloat16().view(torch.int16).numpy().view(np.uint16)
                        same(dec, quant, what + ": FP8 codes do not decode to the quantized values", quant != 0x7FC0)
            # ragged and single-group row counts: the first n rows as their own launch
            fmt, lut, _ = formats[None]
            flat = own.reshape(-1, cols)
            for n in counts:
                if mask_kind == "per_b" or n > (B * H * Q if mask_kind == "none" else Q):
                    continue
                what = f"softmax {n}x{cols} mask={mask_kind}"
                r = launch(lambda g: L.qt_softmax_fq_probs_bf16(sc.data_ptr(), mp, g["out"].ptr, g["probs"].ptr, 1, 1, n, cols, 0, 0, sq, scaling, ctypes.byref(fmt),
                                                                lp(lut), None, None, stream()), {"out": ((n, cols), np.uint16), "probs": ((n, cols), np.uint16)}, what)
                same(r["probs"], flat[:n], what)


def test_softmax_refuses_a_row_past_the_longest(nv):
    L = nv.lib()
    cols = rc.SOFTMAX_REFUSED_COLS
    z = dev(np.zeros((2, cols), np.uint16))
    fmt, lut, _ = softmax_formats(nv)["e4m3"]
    refused(lambda g: L.qt_softmax_fq_bf16(z.data_ptr(), None, g["out"].ptr, 1, 1, 2, cols, 0, 0, 0, 0.125, ctypes.byref(fmt), lp(lut), None, None, stream()),
            {"out": ((2, cols), np.uint16)}, "qt_softmax_fq_bf16 at 4104 columns")
    refused(lambda g: L.qt_softmax_fq_bf16_fp8(z.data_ptr(), None, None, g["out8"].ptr, 1, 1, 2, cols, 0, 0, 0, 0.125, ctypes.byref(fmt), stream()),
            {"out8": ((2, cols), np.uint8)}, "qt_softmax_fq_bf16_fp8 at 4104 columns")


@pytest.mark.parametrize("cols", rc.SOFTMAX_LIVE_COLS)
@pytest.mark.parametrize("mask_kind", ["per_bq", "per_b"])
def test_softmax_row_live_shortcut_at_every_row_length(nv, cols, mask_kind):
    """qt_softmax_fq_bf16_fp8_live == qt_softmax_fq_bf16_fp8 off 1024 columns: short rows (row_live forces the 64-lane kernel there) and
    1, 2, 4 and 8 vectors per lane, with NaN planted wherever the shortcut promises not to read (the construction of
    tests/test_gpu_parity.py::test_softmax_row_live_shortcut_changes_nothing).  The shortcut skips whole 512-column pieces, so its
    promise begins at column 512: at 8, 136 and 264 columns there is nothing it may skip, no NaN is planted and the test compares the two
    entry points only; at 520 and beyond every case has rows with planted NaN (asserted)."""
    L = nv.lib()
    scaling = 0.125
    c = rc.softmax_case(cols, scaling, mask_kind)
    B, H, Q = c["B"], c["H"], c["Q"]
    shape = (B, H, Q, cols)
    scores = c["scores"].copy()
    scores[o.canon_nan16(scores) == 0x7FC0] = 0                   # (the NaN regime is the forward test's; here NaN marks what must not be read)
    mask = dev(c["mask"])
    sb, sh, sq = c["strides"]
    mrows = B * (Q if mask_kind == "per_bq" else 1)
    live = torch.empty(mrows, dtype=torch.int32, device="cuda")
    nv.check(L.qt_mask_row_live(mask.data_ptr(), mrows, cols, cols, live.data_ptr(), stream()), "qt_mask_row_live")
    m = o.bf16_to_f32(c["mask"]).reshape(mrows, cols)
    want_live = ((m > -1e30) * np.arange(1, cols + 1)).max(axis=1).astype(np.int32)
    assert np.array_equal(live.cpu().numpy(), want_live)
    lsb, lsq = (Q, 1) if mask_kind == "per_bq" else (1, 0)
    lv = np.broadcast_to(want_live.reshape(B, 1, Q if mask_kind == "per_bq" else 1, 1), (B, H, Q, 1))
    beyond = (np.arange(cols)[None, None, None, :] >= (lv + 511) // 512 * 512) & (lv > 0)
    assert bool(beyond.any()) == (cols > 512)
    poisoned = scores.copy()
    poisoned[beyond] = 0x7FC0
    for d in ("e4m3", "e5m2"):
        fmt = nv.format_for(d)
        s0, s1 = dev(scores), dev(poisoned)
        ref = launch(lambda g: L.qt_softmax_fq_bf16_fp8(s0.data_ptr(), mask.data_ptr(), None, g["out8"].ptr, B, H, Q, cols, sb, sh, sq, scaling, ctypes.byref(fmt),
                                                       stream()), {"out8": (shape, np.uint8)}, "fp8")
        got = launch(lambda g: L.qt_softmax_fq_bf16_fp8_live(s1.data_ptr(), mask.data_ptr(), g["out8"].ptr, B, H, Q, cols, sb, sh, sq, scaling, ctypes.byref(fmt),
                                                            live.data_ptr(), lsb, 0, lsq, stream()), {"out8": (shape, np.uint8)}, "fp8_live")
        same(got["out8"], ref["out8"], f"qt_softmax_fq_bf16_fp8_live {d} {cols} mask={mask_kind}")


# ---- softmax backward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", rc.SOFTMAX_BWD_COLS)
def test_softmax_backward_every_row_length(nv, cols):
    """qt_softmax_backward_chain_bf16 against oracle.softmax_backward at 16, 32 and 64 lanes per row and 1, 2 and 4 vectors per lane: P
    from the oracle's forward, one-hot rows (ds == 0) and uniform rows, dP ~ N(0, 1e-4) and N(0, 1), one and two stages bit-equal to
    their own launches."""
    L = nv.lib()
    _, counts = rc.softmax_rows_per_group(cols)
    for dp_std in (1e-4, 1.0):
        c = rc.softmax_bwd_case(cols, dp_std)
        total = len(c["names"])
        iv = o.softmax_backward(c["dp"], c["p"], c["scaling"])
        for n in (total,) + counts:
            dp, p = dev(c["dp"][:n]), dev(c["p"][:n])
            for nstage, scales, src in ((1, (dp_std * 2.0 ** -12,), (-1,)), (2, (dp_std * 2.0 ** -12, dp_std * 2.0 ** -13), (-1, 0))):
                st = Stages(nv, "fp8_e5m2", scales, src, (n, cols))
                what = f"qt_softmax_backward_chain_bf16 {n}x{cols} dP~N(0,{dp_std}) {nstage} stage(s)"
                r = launch(lambda g: L.qt_softmax_backward_chain_bf16(dp.data_ptr(), p.data_ptr(), g["ds"].ptr, n, cols, c["scaling"], st.array(g), nstage,
                                                                     ctypes.byref(st.fmt), st.lut.data_ptr(), stream()), {"ds": ((n, cols), np.uint16), **st.specs()}, what)
                inside(iv.rows(slice(0, n)), r["ds"], what, "softmax_backward")
                st.check(r, r["ds"], what)


def test_softmax_backward_refuses_a_row_past_the_longest(nv):
    L = nv.lib()
    cols = rc.SOFTMAX_BWD_REFUSED_COLS
    z = dev(np.zeros((2, cols), np.uint16))
    st = Stages(nv, "fp8_e5m2", (1.0,), (-1,), (2, cols))
    refused(lambda g: L.qt_softmax_backward_chain_bf16(z.data_ptr(), z.data_ptr(), g["ds"].ptr, 2, cols, 0.125, st.array(g, zero=False), 1, ctypes.byref(st.fmt),
                                                      st.lut.data_ptr(), stream()), {"ds": ((2, cols), np.uint16), **st.specs()},
            "qt_softmax_backward_chain_bf16 at 2056 columns")


# ---- causal-LM loss ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rc.LOSS_SHAPES)
def test_causal_lm_loss_rows_and_mean(nv, shape):
    """qt_causal_lm_loss_bf16 against oracle.causal_lm_nll: a vocabulary shorter than one vector, exactly one vector, a non-vector tail
    behind 256 vectors, a second trip of the lane loop, and one position (nothing scored: NaN).  The per-row losses are read from the
    scratch rows: -1 exactly where a row is not scored, the others and the mean within their radii."""
    L = nv.lib()
    B, S, V, stride = shape
    for regime in rc.LOSS_REGIMES:
        c = rc.loss_case(shape, regime)
        if c is None:
            continue
        logits, labels = dev(c["logits"]), dev(c["labels"])
        what = f"qt_causal_lm_loss_bf16 {shape} {regime}"
        r = launch(lambda g: L.qt_causal_lm_loss_bf16(logits.data_ptr(), labels.data_ptr(), B, S, V, stride, -100, g["rows"].ptr, g["loss"].ptr, stream()),
                   {"rows": ((B, S), np.float32), "loss": ((1,), np.float32)}, what)
        loss, rho, scored, mean, rho_mean = o.causal_lm_nll(c["logits"][..., :V], c["labels"])
        got = r["rows"].astype(np.float64)
        assert np.array_equal(got == -1.0, ~scored), what + ": the -1 marks"
        nan = np.isnan(loss) & scored
        assert np.array_equal(np.isnan(got), nan), what + ": NaN rows"
        fin = scored & ~nan
        worst = float(np.max(np.abs(got[fin] - loss[fin]) / rho[fin])) if fin.any() else 0.0
        s = STATS.setdefault("causal_lm_loss (distance / radius)", [1.0, 0.0])
        s[1] = max(s[1], worst)
        assert worst <= 1.0, f"{what}: a row loss is {worst:.3f} radii from the oracle"
        if np.isnan(mean):
            assert np.isnan(r["loss"][0]), what
        else:
            assert abs(float(r["loss"][0]) - mean) <= rho_mean, f"{what}: mean {float(r['loss'][0])!r} vs {mean!r} +- {rho_mean:.3g}"
