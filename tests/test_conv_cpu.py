"""QAT convolutions on the CPU: the Conv / ConvBn twins against traces of upstream's (tests/golden/conv_traces.*, conv_cnn.*; generator:
tests/golden/gen_golden_conv.py, whose model, input and driver helpers run here against this package)."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.ao.nn.intrinsic as nni
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, G)
import gen_golden_conv as gc  # noqa: E402

import quantized_training as qt  # noqa: E402
from quantized_training.modules import qat as nnqat  # noqa: E402
from quantized_training.qconfig import get_qconfig  # noqa: E402
from quantized_training.quantization_mappings import DEFAULT_QAT_MODULE_MAPPINGS  # noqa: E402


def _make_args(**kw):
    a = qt.add_qspec_args().parse_args([])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


IMPL = gc.Impl(nnqat, get_qconfig, qt.quantize, _make_args)


@pytest.fixture(scope="module")
def traces():
    npz = np.load(os.path.join(G, "conv_traces.npz"))
    with open(os.path.join(G, "conv_traces.json")) as f:
        return npz, json.load(f)


@pytest.fixture(scope="module")
def cnn():
    npz = np.load(os.path.join(G, "conv_cnn.npz"))
    with open(os.path.join(G, "conv_cnn.json")) as f:
        return npz, json.load(f)


def _get(npz, key, dtype):
    return gc.from_bits(npz[key.replace("/", "__")], getattr(torch, dtype))


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(gc.bits(a), gc.bits(b)), what


# ---- 1. mappings and exports ---------------------------------------------------------------------------------------------------------
def test_mappings_and_exports():
    for flt, twin in ((nn.Conv2d, "Conv2d"), (nn.Conv3d, "Conv3d"), (nni.ConvBn1d, "ConvBn1d"), (nni.ConvBn2d, "ConvBn2d"),
                      (nni.ConvBn3d, "ConvBn3d")):
        assert DEFAULT_QAT_MODULE_MAPPINGS[flt] is getattr(nnqat, twin)
    assert nn.Conv1d not in DEFAULT_QAT_MODULE_MAPPINGS                # (upstream does not map it either)
    assert DEFAULT_QAT_MODULE_MAPPINGS[nn.Linear] is nnqat.Linear
    for name in ("Conv1d", "Conv2d", "Conv3d", "ConvBn1d", "ConvBn2d", "ConvBn3d"):
        assert isinstance(getattr(nnqat, name), type)
    assert callable(nnqat.update_bn_stats) and callable(nnqat.freeze_bn_stats)


# ---- 2. quantize() on the mini CNN ---------------------------------------------------------------------------------------------------
def test_quantize_mini_cnn_structure(cnn):
    _, meta = cnn
    m = gc.build_cnn(IMPL)
    assert [[n, type(mod).__name__] for n, mod in m.named_modules()] == meta["modules"]
    assert sorted(m.state_dict().keys()) == meta["state_dict_keys"]
    assert any(k.startswith("c2.weight_fake_quant.") for k in m.state_dict())


# ---- 3. module traces ----------------------------------------------------------------------------------------------------------------
def _inputs(npz, key):
    return [_get(npz, f"{key}/x{i}", "bfloat16") for i in range(gc.N_CALLS)]


def _check_calls(npz, meta, key, calls, exact_out, close_out=False):
    dt = meta[key]["dtypes"]
    for i, rec in enumerate(calls):
        for name in ("wq", "scale", "amax_history"):
            _same_bits(rec[name], _get(npz, f"{key}/call{i}/{name}", dt[name]), (key, i, name))
        want = _get(npz, f"{key}/call{i}/out", dt["out"])
        if exact_out:
            _same_bits(rec["out"], want, (key, i, "out"))
        elif close_out:
            torch.testing.assert_close(rec["out"], want)


@pytest.mark.parametrize("spec", list(gc.SPECS))
@pytest.mark.parametrize("name", list(gc.LAYERS))
def test_conv_trace(traces, spec, name):
    """Quantized weight, scale and amax history bit for bit; the output bit for bit in the exact tier (int8, power-of-two scales,
    K <= 1024: every dot product is exact in fp32 whatever its order) and against the fp64 convolution elsewhere (item 4)."""
    npz, meta = traces
    key = f"{spec}/{name}"
    xs = _inputs(npz, key)
    m = gc.build_layer(IMPL, spec, name)
    calls = gc.run_trace(m, xs)
    _check_calls(npz, meta, key, calls, exact_out=spec == "int8_pow2" and m.bias is None)
    for x, rec in zip(xs, calls):
        _check_bound(m, x, rec["wq"], rec["out"])
    f = m.to_float()
    assert type(f) is getattr(nn, gc.LAYERS[name][0]) and torch.equal(f.weight, m.weight)


def _conv_fn(mod):
    return {3: F.conv1d, 4: F.conv2d, 5: F.conv3d}[mod.weight.dim()]


def _check_bound(mod, x, wq, y, bias=True):
    """|y - ref| <= 2^-8 |ref| + 2^-18 conv(|x|, |wq|), ref the fp64 convolution of the quantized operands (the bound of the project's
    bf16 GEMMs, tests/test_gpu_parity.py::test_train_gemm_against_fp64_products)."""
    conv = _conv_fn(mod)
    kw = dict(stride=mod.stride, padding=mod.padding, dilation=mod.dilation, groups=mod.groups)
    b = mod.bias.double() if bias and mod.bias is not None else None
    ref = conv(x.double(), wq.double(), b, **kw)
    mag = conv(x.double().abs(), wq.double().abs(), None if b is None else b.abs(), **kw)
    err = (y.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -18 * mag
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"conv bound: worst err / bound = {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("spec", list(gc.SPECS))
@pytest.mark.parametrize("mode", list(gc.CONVBN_MODES))
def test_convbn_trace(traces, spec, mode):
    npz, meta = traces
    key = f"{spec}/convbn2d/{mode}"
    dt = meta[key]["dtypes"]
    xs = _inputs(npz, f"{spec}/convbn2d")
    m = gc.build_convbn(IMPL, spec, mode)
    assert m.bn.training == meta[key]["bn_training"] and m.training == meta[key]["training"]

    def load_bn(i, mod):
        # every call starts from upstream's BN buffers: a last-bit difference of a running variance (torch's training-mode batch norm is
        # a reduction neither side controls) must not move the next call's weight codes
        for b in gc.BN_BUFFERS:
            getattr(mod.bn, b).copy_(_get(npz, f"{key}/call{i}/bn_before.{b}", dt["bn_before." + b]))

    calls = gc.run_trace(m, xs, load_bn if mode == "train_update" else None)
    elementwise_after_conv = mode != "train_update"
    _check_calls(npz, meta, key, calls, exact_out=spec == "int8_pow2" and elementwise_after_conv, close_out=True)
    for i, rec in enumerate(calls):
        for b in gc.BN_BUFFERS:
            want = _get(npz, f"{key}/call{i}/bn_after.{b}", dt["bn_after." + b])
            assert rec["bn_after." + b].shape == want.shape and rec["bn_after." + b].dtype == want.dtype
            if mode == "train_update" and b != "num_batches_tracked":
                torch.testing.assert_close(rec["bn_after." + b], want)
            else:
                _same_bits(rec["bn_after." + b], want, (key, i, b))
    assert sorted(k for k in m.state_dict() if k.startswith("bn.")) == sorted("bn." + b for b in gc.BN_BUFFERS + ("weight", "bias"))
    if mode == "train_frozen":
        f = m.to_float()
        assert type(f).__name__ == meta[key]["to_float"]
        _same_bits(f.weight.detach(), _get(npz, f"{key}/to_float.weight", "bfloat16"), "to_float.weight")
        _same_bits(f.bias.detach(), _get(npz, f"{key}/to_float.bias", "bfloat16"), "to_float.bias")


def test_convbn_train_keeps_a_frozen_bn_and_slow_path_runs():
    m = gc.build_convbn(IMPL, "int8_pow2", "train_frozen")
    m.eval()
    m.train()
    assert m.training and not m.bn.training
    m.apply(nnqat.update_bn_stats)
    assert m.bn.training and not m.freeze_bn
    m.apply(nnqat.freeze_bn_stats)
    assert not m.bn.training and m.freeze_bn
    x = gc.activation_inputs(IMPL, "int8_pow2", gc.CONVBN_INPUT, 5)[0]
    with torch.no_grad():
        m(x), m(x)                                        # (delayed scaling: the first calls still quantize with the initial scale)
        m.weight_fake_quant.disable_observer()
        fast = m(x)
        m._enable_slow_path_for_better_numerical_stability = True
        slow = m(x)
        m.update_bn_stats()
        assert m(x).shape == fast.shape
    # frozen: both paths are conv(x, fq(W s)) / s ... bn(...) resp. conv(...) + fused bias -- equal up to bf16 rounding of the chain
    torch.testing.assert_close(slow.float(), fast.float(), atol=0.25, rtol=0.05)


def test_from_float_unwraps_fused_and_builds_real_quantizer_buffers():
    conv = nn.Conv2d(8, 8, 3)
    conv.qconfig = gc.qconfig_of(IMPL, "e4m3")
    twin = nnqat.Conv2d.from_float(conv)
    assert twin.weight is conv.weight and twin.bias is conv.bias
    assert all(b.device.type == "cpu" for b in twin.weight_fake_quant.buffers())
    assert not any(p.is_meta for p in twin.parameters())
    with pytest.raises(AssertionError):
        nnqat.Conv3d.from_float(conv)


# ---- 4. tolerance tier: large contractions, operands drawn here ----------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["e4m3", "posit8_1"])
@pytest.mark.parametrize("shape", [(1, 512, 6, 6, 16, 3, 1, 1), (2, 512, 5, 5, 32, 1, 1, 0), (1, 64, 9, 9, 16, 4, 1, 0), (1, 128, 8, 8, 16, 3, 2, 1)])
def test_conv2d_large_k_bound(spec, shape):
    n, cin, h, w, cout, k, stride, pad = shape
    conv = gc.seed_params_(nn.Conv2d(cin, cout, k, stride=stride, padding=pad, bias=False), 11).bfloat16()
    conv.qconfig = gc.qconfig_of(IMPL, spec)
    m = nnqat.Conv2d.from_float(conv)
    x = gc.activation_inputs(IMPL, spec, (n, cin, h, w), 91)[0]
    rec = gc.run_trace(m, [x])[0]
    _check_bound(m, x, rec["wq"], rec["out"])


# ---- 5. checkpoints ------------------------------------------------------------------------------------------------------------------
def test_reference_checkpoint_loads_and_reproduces_logits(cnn):
    npz, meta = cnn
    m = gc.build_cnn(IMPL)
    sd = {k: _get(npz, "sd/" + k, dt) for k, (_, dt) in meta["state_dict"].items()}
    # upstream's flow, as in test_blocks_golden.test_upstream_checkpoint_loads_and_reproduces: one forward (on other data than the
    # checkpoint saw) registers the activation fake-quantizers, then the checkpoint is loaded over whatever state that left
    with torch.no_grad():
        m(gc.rand_bf16(999, gc.CNN_INPUT) * 3.0)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    for k, v in m.state_dict().items():
        _same_bits(v, sd[k], k)
    gc.freeze_for_eval(m)
    with torch.no_grad():
        y = m(_get(npz, "eval/x", "bfloat16"))
    _same_bits(y, _get(npz, "eval/logits", meta["eval_dtype"]), "eval logits")


def test_v1_named_convbn_state_dict_loads():
    m = gc.build_convbn(IMPL, "int8_pow2", "train_update")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    v1 = {}
    rename = {"bn.weight": "gamma", "bn.bias": "beta", "bn.running_mean": "running_mean", "bn.running_var": "running_var",
              "bn.num_batches_tracked": "num_batches_tracked"}
    for k, v in sd.items():
        v1[rename.get(k, k)] = v + 1 if k in ("bn.weight", "bn.running_mean") else v
    v1 = {k: v for k, v in v1.items()}
    m2 = gc.build_convbn(IMPL, "int8_pow2", "train_update")
    meta_sd = torch.nn.modules.module.OrderedDict(v1)
    meta_sd._metadata = {"": {"version": 1}}
    m2.load_state_dict(meta_sd, strict=True)
    assert torch.equal(m2.bn.weight, sd["bn.weight"] + 1) and torch.equal(m2.bn.running_mean, sd["bn.running_mean"] + 1)
    assert torch.equal(m2.bn.running_var, sd["bn.running_var"])


# ---- the route rule (pure host logic; the device side is tests/test_gpu_conv.py) ------------------------------------------------------------
def test_auto_route_rule_and_cpu_tensors_stay_on_torch(monkeypatch):
    from quantized_training import conv_route
    # (output pixels, k tiles) of ResNet-50 body layers at batch 32, by what profiles/conv2d_routes.txt measured
    assert conv_route._auto_takes(32 * 56 * 56, 9) and conv_route._auto_takes(32 * 7 * 7, 72)         # 3 x 3
    assert conv_route._auto_takes(32 * 28 * 28, 8) and conv_route._auto_takes(32 * 14 * 14, 4)        # 1 x 1, Cin 512 / Cin 256 on 14 x 14
    assert not conv_route._auto_takes(32 * 56 * 56, 1) and not conv_route._auto_takes(32 * 28 * 28, 2) and not conv_route._auto_takes(32 * 56 * 56, 4)
    for mode, want in (("0", "0"), ("1", "1"), ("auto", "auto"), ("yes", "auto")):
        monkeypatch.setenv("QT_CONV_GEMM", mode)
        assert conv_route.conv_gemm_mode() == want
    monkeypatch.delenv("QT_CONV_GEMM")
    assert conv_route.conv_gemm_mode() == "auto"
    assert conv_route._resolve_padding("valid", (3, 3), (1, 1), (1, 1)) == (0, 0)
    assert conv_route._resolve_padding("same", (3, 5), (1, 1), (2, 1)) == (2, 2)
    assert conv_route._resolve_padding("same", (4, 3), (1, 1), (1, 1)) is None                          # torch pads one side more
    monkeypatch.setenv("QT_CONV_GEMM", "1")
    before = dict(conv_route.CONV_ROUTES)
    assert conv_route.conv2d_or_none(torch.zeros(1, 64, 4, 4).bfloat16(), torch.zeros(8, 64, 1, 1).bfloat16(), None, (1, 1), (0, 0), (1, 1), 1) is None
    assert conv_route.CONV_ROUTES == before                                                           # CPU tensors never touch the route
