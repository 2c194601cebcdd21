"""record_histogram without a GPU (quantized_training/histogram.py, csrc/qt_histogram.hip): the new C symbols, the closed form the kernel
counts by against the reference's composite on every bf16 and fp16 pattern, why fp32 is declined, every decline of the router, the
switch, and the grouping / plotting functions the reference's examples import."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["qt_exp_histogram_bf16", "qt_exp_histogram_f16", "qt_exp_histogram_plan", "qt_fake_quant_hist_bf16"]


def composite(x):
    """The reference's two lines (fake_quantize.py:348-350) into a fresh buffer."""
    exp = torch.floor(torch.log2(torch.abs(x.detach().float())))
    return torch.histc(exp, 254, min=-126, max=127)


def closed_form(x):
    """What the kernel counts: the exponent field E of the exact fp32 image, 1 <= E <= 254 into bin E - 1."""
    E = (x.detach().float().contiguous().view(torch.int32).numpy().view(np.uint32).reshape(-1) >> 23) & 0xFF
    return np.bincount(E, minlength=256)[1:255].astype(np.float32)


def all_patterns(dtype):
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_in_header_and_native_table(name):
    from quantized_training import _native
    with open(os.path.join(ROOT, "include", "qt_hip.h")) as f:
        header = f.read()
    assert re.search(rf"\bint {name}\(", header), name
    assert name in _native.SIGNATURES
    assert _native.ABI_VERSION == 3 and "#define QT_ABI_VERSION 3" in header
    args = _native.SIGNATURES[name][1]
    assert len(args) == {"qt_exp_histogram_bf16": 6, "qt_exp_histogram_f16": 6, "qt_exp_histogram_plan": 2, "qt_fake_quant_hist_bf16": 11}[name]


def test_public_exports():
    import quantized_training as qt
    from quantized_training import histogram
    for name in ("get_grouped_histogram", "plot_histogram", "plot_layer_range"):
        assert getattr(qt, name) is getattr(histogram, name) and name in qt.__all__


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_closed_form_equals_composite_on_every_pattern(dtype):
    x = all_patterns(dtype)
    # one pattern at a time: a bin per pattern, or none
    exp = torch.floor(torch.log2(torch.abs(x.float())))
    E = (x.float().view(torch.int32).numpy().view(np.uint32) >> 23) & 0xFF
    counted = (E >= 1) & (E <= 254)
    ref = exp.numpy()
    in_range = np.isfinite(ref) & (ref >= -126) & (ref <= 127)
    assert np.array_equal(counted, in_range)
    assert np.array_equal((E[counted] - 1).astype(np.int64), (ref[counted] + 126).astype(np.int64))
    for i in np.flatnonzero(~counted)[::97]:                      # histc itself counts none of them (zeros, subnormal-as-fp32, inf, NaN)
        assert float(composite(x[i:i + 1]).sum()) == 0.0, i
    # the tensor holding every pattern once
    got, want = closed_form(x), composite(x).numpy()
    assert np.array_equal(got, want)
    if dtype == torch.bfloat16:
        assert np.all(got == 256.0)                               # 2 signs x 128 mantissas in each of the 254 bins
    else:
        assert got[102:112].tolist() == [2.0 * (1 << k) for k in range(10)]      # fp16 subnormals: m 2^-24, bins 102..111
        assert np.all(got[112:142] == 2048.0) and got[:102].sum() == 0 and got[142:].sum() == 0


def test_fp32_counter_example_is_why_fp32_is_declined():
    """2^k minus one ulp: floor(log2f(x)) says k for most k, the exponent field says k - 1."""
    k = np.arange(-125, 128)
    below = np.nextafter(np.exp2(k.astype(np.float64)).astype(np.float32), np.float32(0))
    x = torch.from_numpy(below)
    by_field = ((below.view(np.uint32) >> 23) & 0xFF).astype(np.int64) - 127
    assert np.array_equal(by_field, k - 1)
    by_log2 = torch.floor(torch.log2(x)).numpy().astype(np.int64)
    up = int((by_log2 == k).sum())
    assert up >= 200 and np.all((by_log2 == k) | (by_log2 == k - 1)), up     # the library's log2f rounds up for most of them
    assert not np.array_equal(closed_form(x), composite(x).numpy())


def _fq(**kw):
    import quantized_training as qt
    from dataclasses import asdict
    spec = asdict(qt.QuantizationSpec.from_str(kw.pop("spec", "e4m3")))
    return qt.FusedAmaxObsFakeQuantize(**spec, record_histogram=True, **kw)


def _cases():
    g = torch.Generator().manual_seed(3)
    base = torch.randn(6, 40, generator=g) * 3
    yield "cpu bf16", base.bfloat16(), torch.zeros(254)
    yield "cpu fp16", base.half(), torch.zeros(254)
    yield "cpu fp32", base, torch.zeros(254)
    yield "bf16 histogram buffer", base.bfloat16(), torch.zeros(254, dtype=torch.bfloat16)
    yield "overlapping view", base.bfloat16().as_strided((6, 40), (20, 1)), torch.zeros(254)
    yield "expanded view", base.bfloat16()[:1].expand(6, 40), torch.zeros(254)
    yield "permuted view", base.bfloat16().t(), torch.zeros(254)
    yield "empty", base.bfloat16()[:0], torch.zeros(254)


@pytest.mark.parametrize("case", list(_cases()), ids=[c[0] for c in _cases()])
def test_router_declines_run_the_composite_bit_for_bit(case):
    from quantized_training import histogram
    _, x, hist = case
    hist += 0.5
    want = hist.clone()
    want += composite(x)
    histogram.reset_stats()
    assert histogram.exp_histogram_or_none(x, hist) is None and histogram.fused_state(x, hist) is None
    histogram.record(x, hist)
    assert histogram.STATS == {"histogram_native": 0, "histogram_fused": 0, "histogram_composite": 1}
    assert torch.equal(hist, want)


def test_eligibility_rule_on_meta_tensors(monkeypatch):
    """The rule itself, device cases included, without a device: meta tensors carry dtype, shape and strides."""
    from quantized_training import histogram
    monkeypatch.delenv("QT_HISTOGRAM", raising=False)

    class Dev:                                                     # a stand-in whose device says "cuda"
        def __init__(self, t, index=0):
            self.t, self.device = t, torch.device("cuda", index)
            self.dtype, self.shape = t.dtype, t.shape

        def __getattr__(self, name):
            return getattr(self.t, name)

    def x(dtype=torch.bfloat16, shape=(4, 8), strides=None):
        t = torch.empty(shape, dtype=dtype, device="meta")
        return Dev(t if strides is None else t.as_strided(shape, strides))

    hist = Dev(torch.empty(254, device="meta"))
    assert histogram.eligible(x(), hist) and histogram.eligible(x(torch.float16), hist)
    assert histogram.eligible(x(strides=(1, 4)), hist)                                  # dense in another order
    assert histogram.eligible(x(shape=(2, 1, 8), strides=(8, 99, 1)), hist)            # a size-1 dimension's stride does not matter
    assert not histogram.eligible(x(torch.float32), hist)
    assert not histogram.eligible(x(strides=(16, 1)), hist)                             # gaps
    assert not histogram.eligible(x(strides=(4, 1)), hist)                              # overlapping
    assert not histogram.eligible(x(strides=(0, 1)), hist)
    assert not histogram.eligible(x(), Dev(torch.empty(254, dtype=torch.bfloat16, device="meta")))
    assert not histogram.eligible(x(), Dev(torch.empty(255, device="meta")))
    assert not histogram.eligible(x(), Dev(torch.empty(508, device="meta")[::2]))
    assert not histogram.eligible(x(), Dev(torch.empty(254, device="meta"), index=1))   # another device
    assert not histogram.eligible(x(shape=(1 << 16, 1 << 16)), hist)                    # 2^32 elements: counts are u32
    assert histogram.eligible(x(shape=((1 << 16) - 1, 1 << 16)), hist)
    monkeypatch.setenv("QT_HISTOGRAM", "0")
    assert not histogram.eligible(x(), hist)


def test_switch_is_declared_once_and_read_at_call_time(monkeypatch):
    from quantized_training import switches
    assert switches.SWITCHES["QT_HISTOGRAM"][:2] == ("1", switches.ON)
    for value, want in ((None, True), ("", True), ("0", False), ("1", True), ("junk", True)):
        if value is None:
            monkeypatch.delenv("QT_HISTOGRAM", raising=False)
        else:
            monkeypatch.setenv("QT_HISTOGRAM", value)
        assert switches.on("QT_HISTOGRAM") is want, value


@pytest.mark.parametrize("spec", ["e4m3", "int8,qs=per_tensor_symmetric", "posit8_1"])
def test_module_on_cpu_is_the_reference_sequence(spec):
    from quantized_training import histogram
    m = _fq(spec=spec)
    g = torch.Generator().manual_seed(5)
    want = torch.zeros(254)
    histogram.reset_stats()
    for scale in (1.0, 30.0, 1e-3):
        x = (torch.randn(7, 96, generator=g) * scale).bfloat16()
        m(x)
        want += composite(x)
    assert torch.equal(m.histogram, want) and histogram.STATS["histogram_composite"] == 3


class _Toy(torch.nn.Module):
    """Names of both shapes: `layer.N.<layer>.activation_pre_process.K` and a quantizer with no numbered block in front."""

    def __init__(self):
        super().__init__()
        import quantized_training as qt

        def fq():
            return qt.FusedAmaxObsFakeQuantize("e4m3", record_histogram=True)

        def hooked(*names):
            mod = torch.nn.Module()
            for n in names:
                sub = torch.nn.Module()
                sub.activation_pre_process = torch.nn.ModuleList([fq()])
                mod.add_module(n, sub)
            return mod
        self.layer = torch.nn.ModuleList([hooked("query", "dense"), hooked("query", "dense")])
        self.classifier = torch.nn.Module()
        self.classifier.activation_pre_process = torch.nn.ModuleList([fq()])
        self.weight_fake_quant = fq()


def _filled_toy():
    torch.manual_seed(0)
    toy = _Toy()
    for i, (_, m) in enumerate((n, m) for n, m in toy.named_modules() if hasattr(m, "histogram")):
        for _ in range(2):
            m((torch.randn(64, 64) * 2.0 ** (i - 3)).bfloat16())
    return toy


def test_get_grouped_histogram_groups_both_name_shapes():
    import quantized_training as qt
    toy = _filled_toy()
    groups = qt.get_grouped_histogram(toy)
    assert {k: [n for n, _ in v] for k, v in groups.items()} == {
        "layer.0": ["query", "dense"], "layer.1": ["query", "dense"], "classifier": ["classifier"], "weight_fake_quant": ["weight_fake_quant"]}
    h = groups["layer.1"][0][1]
    assert isinstance(h, np.ndarray) and h.shape == (254,) and h.sum() > 0
    assert np.array_equal(h, toy.layer[1].query.activation_pre_process[0].histogram.numpy())


def test_plots_write_the_expected_files(tmp_path):
    import quantized_training as qt
    toy = _filled_toy()
    qt.plot_histogram(toy, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["classifier.png", "layer.0.png", "layer.1.png", "weight_fake_quant.png"]
    qt.plot_layer_range(toy, str(tmp_path))
    assert "layer_distribution.png" in os.listdir(tmp_path)
    for name in os.listdir(tmp_path):
        with open(tmp_path / name, "rb") as f:
            assert f.read(8) == b"\x89PNG\r\n\x1a\n", name


def test_importing_the_package_does_not_import_matplotlib():
    """(scipy is not asked about: torch's own imports may bring it in.  histogram.py imports both inside the plotting functions only.)"""
    code = ("import sys; sys.path[:0] = [%r, %r]; import quantized_training; "
            "print(int('matplotlib' in sys.modules))" % (ROOT, os.path.join(ROOT, "quantized-training_amd")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0"], out
    import ast
    with open(os.path.join(ROOT, "quantized-training_amd", "quantized_training", "histogram.py")) as f:
        tree = ast.parse(f.read())
    top = {a.name.split(".")[0] for n in tree.body if isinstance(n, ast.Import) for a in n.names}
    top |= {n.module.split(".")[0] for n in tree.body if isinstance(n, ast.ImportFrom) and n.module}
    assert not top & {"matplotlib", "scipy"}, top
