"""Every QT_* environment switch, declared once: name -> (default, kind, category, meaning).  A leaf module.  Each accessor reads os.environ
when it is called (nothing is cached: a switch may be flipped in mid-process); an unknown name raises KeyError.  README.md's table is
checked against this one (tests/test_switches_cpu.py).
kinds       ON: on unless "0" | OFF: off unless "1" | TRI: "auto" / "0" / "1", anything else counts as "auto" |
            LEVEL: "0" / "1" / "2", anything else counts as "1" | MASK: an integer in any base Python reads | RAW: the string itself
categories  product: read by the package | native: read by libqt_hip.so | bench: read by bench.py   (the last two: listed only) |
            option: read by the package too -- the route of a per-call quantizer option, added after the 27 `product` switches whose
            names tests/test_switches_cpu.py pins"""
import os

ON, OFF, TRI, LEVEL, MASK, RAW = "on", "off", "tri", "level", "mask", "raw"

SWITCHES = {
    "QT_FP8_GEMM": ("1", ON, "product", "E4M3 / E5M2 layers multiply FP8 codes (else the bf16 GEMM route)"),
    "QT_FQ8_GEMM": ("auto", TRI, "product", "weight fake-quant inside the FP8 GEMM: by the route table / never / always"),
    "QT_FQ8_MLP": ("1", LEVEL, "product", "gate + up + SiLU*up as one launch: never / by the table / always"),
    "QT_FQT_GEMM": ("auto", TRI, "product", "value map inside a bf16 GEMM for non-FP8 Linears: by the route rule / never / always"),
    "QT_LT_GEMM": ("1", ON, "product", "FP8 library GEMMs through the directly driven hipBLASLt (else torch._scaled_mm)"),
    "QT_LT_ALGO": (None, RAW, "product", "tools only: run hipBLASLt's i-th suggestion whatever the committed table says"),
    "QT_SIBLING_GEMM": ("1", ON, "product", "q / k / v projections as one launch"),
    "QT_GATE_UP_GROUP": ("1", ON, "product", "gate and up of a value-map MLP as one launch"),
    "QT_FUSED_GEMM": ("0", OFF, "product", "round 1's bf16 GEMM with the weight fake-quantized while staged, for every Linear"),
    "QT_FUSED_SOFTMAX": ("1", ON, "product", "scaling, mask, softmax and the probabilities' fake-quant as one pass"),
    "QT_FUSED_ATTENTION": ("auto", TRI, "product", "single-launch attention kernel: where it measured faster / never / always"),
    "QT_FP8_ATTENTION": ("1", ON, "product", "Q.K^T and P.V on FP8 codes (else bf16 GEMMs)"),
    "QT_FP8_ATTENTION_KERNEL": ("1", ON, "product", "qt_attention_fp8 (else the GEMM -> score pass -> GEMM chain)"),
    "QT_ROPE_VALUE_LAUNCH": ("1", ON, "product", "the attention kernel's value pass rides in the rotary launch"),
    "QT_ROPE_WEIGHT_PASS": ("1", ON, "product", "the output projection's weight pass rides in the rotary launch"),
    "QT_FUSED_MODEL_OPS": ("1", ON, "product", "one-launch RMSNorm / rotary / SiLU*up / LayerNorm / GELU (else Hugging Face's chains)"),
    "QT_FUSED_PRODUCER_FQ": ("1", ON, "product", "producer kernels apply the consumer's fake-quantizer"),
    "QT_FUSED_PRODUCER_MAP": ("1", ON, "product", "the same for table formats (row form)"),
    "QT_CODES_ONLY": ("1", ON, "product", "producers write only the FP8 codes where the consumer multiplies codes"),
    "QT_LAZY_POISON": ("0", OFF, "product", "fill the tensors a codes-only producer leaves unwritten with NaN (the tests set it)"),
    "QT_PT2E_FUSE": ("1", ON, "product", "launch fusions on prepared PT2E graphs of device models"),
    "QT_PT2E_NATIVE": ("1", ON, "product", "converted PT2E per-tensor graphs run the native int8 / FP8 GEMM ops"),
    "QT_MX_GEMM": ("1", ON, "product", "block-scaled GEMMs, conv2d_mx and the outlier side path on the in-tree kernels (else the reference formulation)"),
    "QT_TRAIN_DEBUG": ("0", MASK, "product", "training step: bits that switch a fusion OFF (train_fusions.DEBUG_BITS)"),
    "QT_CONV_GEMM": ("auto", TRI, "product", "in-tree implicit-GEMM Conv2d: by the committed rule / never / wherever it applies"),
    "QT_TRAIN_GEMM": ("1", ON, "product", "training step: a QAT Linear's three products on qt_train_gemm_bf16 (else torch's GEMMs)"),
    "QT_HIP_LIB": (None, RAW, "product", "tools only: load another build of the library"),
    "QT_HISTOGRAM": ("1", ON, "option", "record_histogram on bf16 / fp16 device tensors as one HIP launch (else the torch composite)"),
    "QT_MX_WIDE": (None, RAW, "native", "test hook: force the 128 x 128 / the wide block-scaled kernel"),
    "QT_MX_WIDE_TM": (None, RAW, "native", "test hook: the wide block-scaled kernel's tile height"),
    "QT_BENCH_DROPOUT": (None, RAW, "bench", "bench.py, training workload: another dropout probability"),
    "QT_BENCH_NO_OBSERVE": (None, RAW, "bench", "bench.py, training workload: every observer frozen"),
}
_RECOGNISED = {TRI: (("0", "1"), "auto"), LEVEL: (("0", "2"), "1")}
_DEFAULT = {name: row[0] for name, row in SWITCHES.items()}              # (on() runs on every eager forward: two plain look-ups, no more)
_OFF = frozenset(name for name, row in SWITCHES.items() if row[1] == OFF)


def raw(name):
    """The switch's string as set, else its default (None where it has none)."""
    return os.environ.get(name, _DEFAULT[name])


def on(name):
    """ON / OFF switches, and "not switched off" for TRI / LEVEL ones: an ON switch is off only at "0", an OFF switch on only at "1"."""
    v = os.environ.get(name, _DEFAULT[name])
    return v == "1" if name in _OFF else v != "0"


def mode(name):
    """TRI: "auto" | "0" | "1";  LEVEL: "0" | "1" | "2".  An unexpected value counts as the default."""
    values, other = _RECOGNISED[SWITCHES[name][1]]
    v = os.environ.get(name, other)
    return v if v in values else other


def mask(name, bits):
    """MASK: the integer; `bits` (name -> bit) goes into the error text of a value that is no integer."""
    try:
        return int(raw(name) or "0", 0)
    except ValueError:
        raise ValueError(f"{name}={os.environ.get(name)!r}: an integer mask of {bits}") from None
