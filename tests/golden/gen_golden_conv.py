"""Golden fixtures of upstream's QAT convolutions (modules/qat/conv.py, conv_fused.py) -- run by hand in the container that holds the
upstream checkout (`python tests/golden/gen_golden_conv.py`, imports it through _ref_import); tests/test_conv_cpu.py and
tests/test_gpu_conv.py import only the model / input / driver helpers below and run them against this package.

  conv_traces.npz + conv_traces.json
        Conv1d / Conv2d / Conv3d and ConvBn2d (training with the BN updating, training with the BN frozen, eval), three calls each so
        that the delayed-scaling state advances, for int8 per-tensor symmetric with power-of-two scales, e4m3 and posit8_1, in bf16.
        The inputs are what the layer sees under quantize(): outputs of an activation fake-quantizer of the same spec.  Per call: the
        quantized weight (forward hook on weight_fake_quant), scale, amax_history, the output, the BN buffers before and after the call;
        for the frozen ConvBn2d also to_float()'s folded weight and bias.
  conv_cnn.npz + conv_cnn.json
        upstream `quantize(model, args)` on MiniCNN (Conv2d(3, 64) + BN fused by fuse_modules_qat -> ReLU -> Conv2d(64, 64, 3, stride 2)
        -> amax over the plane -> Linear): module class names, the sorted state-dict key list, the state dict after three SGD steps and
        the eval logits (BN frozen, observers disabled) of that checkpoint.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))

SPECS = {
    "int8_pow2": dict(spec="int8,qs=per_tensor_symmetric", pow2=True),
    "e4m3": dict(spec="e4m3", pow2=False),
    "posit8_1": dict(spec="posit8_1", pow2=False),
}

# name: (twin class name, constructor arguments, input shape)
LAYERS = {
    "conv1d": ("Conv1d", dict(in_channels=16, out_channels=24, kernel_size=3, padding=1), (2, 16, 20)),
    "conv2d": ("Conv2d", dict(in_channels=64, out_channels=16, kernel_size=3, padding=1, bias=False), (2, 64, 9, 7)),
    "conv3d": ("Conv3d", dict(in_channels=8, out_channels=16, kernel_size=(2, 3, 3), stride=(1, 2, 1)), (2, 8, 4, 7, 6)),
}
CONVBN = dict(in_channels=64, out_channels=8, kernel_size=3, padding=1, bias=True)
CONVBN_INPUT = (4, 64, 6, 5)
CONVBN_MODES = ("train_update", "train_frozen", "eval")
N_CALLS = 3


# ---- bit-pattern storage -------------------------------------------------------------------------------------------------------------
def bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().astype(np.uint16)
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().astype(np.uint32)
    return t.numpy()


def from_bits(a, dtype):
    if dtype == torch.bfloat16:
        return torch.from_numpy(a.astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16)
    if dtype == torch.float32:
        return torch.from_numpy(a.astype(np.uint32).view(np.int32).copy()).view(torch.float32)
    return torch.from_numpy(a.copy())


def rand_bf16(seed, shape, scale=1.0):
    r = np.random.default_rng(seed)
    return torch.from_numpy((r.standard_normal(shape) * scale).astype(np.float32)).bfloat16()


# ---- what the generator (upstream's classes) and the tests (this package's) both run -------------------------------------------------------
class Impl:
    """The few names the drivers need from an implementation: `nnqat` (the twins), `get_qconfig`, `quantize`, `make_args`."""

    def __init__(self, nnqat, get_qconfig, quantize, make_args):
        self.nnqat, self.get_qconfig, self.quantize, self.make_args = nnqat, get_qconfig, quantize, make_args


def qconfig_of(impl, spec):
    s = SPECS[spec]
    return impl.get_qconfig(s["spec"], s["spec"], None, False, s["pow2"])


def activation_inputs(impl, spec, shape, seed):
    """N_CALLS inputs as a layer sees them under quantize(): a fresh activation fake-quantizer of the spec applied to seeded noise."""
    fq = qconfig_of(impl, spec).activation()
    with torch.no_grad():
        return [fq(rand_bf16(seed + i, shape, 1.0 + 0.5 * i)).clone() for i in range(N_CALLS)]


def seed_params_(mod, seed):
    """Deterministic parameters, and BN statistics that are not the identity, independent of torch's RNG."""
    with torch.no_grad():
        for i, (name, p) in enumerate(sorted(mod.named_parameters())):
            p.copy_(rand_bf16(seed + 7 * i, tuple(p.shape), 0.25).to(p.dtype))
        for name, m in mod.named_modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                m.weight.copy_((rand_bf16(seed + 105, tuple(m.weight.shape)).abs() * 0.5 + 0.5).to(m.weight.dtype))
                m.running_var.copy_((rand_bf16(seed + 101, tuple(m.running_var.shape)).abs() + 0.5).to(m.running_var.dtype))
                m.running_mean.copy_(rand_bf16(seed + 103, tuple(m.running_mean.shape), 0.1).to(m.running_mean.dtype))
    return mod


def build_layer(impl, spec, name, device=None):
    """The twin as quantize() makes it: from_float of a bf16 float layer that carries the qconfig."""
    cls, kw, _ = LAYERS[name]
    flt = seed_params_(getattr(nn, cls)(**kw), 1000 + sorted(LAYERS).index(name)).bfloat16().train()
    flt.qconfig = qconfig_of(impl, spec)
    m = getattr(impl.nnqat, cls).from_float(flt)
    assert m.weight is flt.weight and m.bias is flt.bias
    return m if device is None else m.to(device)


def build_convbn(impl, spec, mode, device=None):
    import torch.ao.nn.intrinsic as nni
    flt = seed_params_(nni.ConvBn2d(nn.Conv2d(**CONVBN), nn.BatchNorm2d(CONVBN["out_channels"])), 2000).bfloat16().train()
    flt.qconfig = qconfig_of(impl, spec)
    m = impl.nnqat.ConvBn2d.from_float(flt)
    assert m.weight is flt[0].weight and m.bn.weight is flt[1].weight and m.bn.running_var is flt[1].running_var
    if mode == "train_frozen":
        m.freeze_bn_stats()
    elif mode == "eval":
        m.eval()
    return m if device is None else m.to(device)


BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def run_trace(mod, inputs, load_bn_before=None):
    """Calls `mod` on every input; per call the quantized weight as weight_fake_quant returned it, its state, the output and, for a fused
    twin, the BN buffers before and after.  `load_bn_before(i, mod)` may set the BN buffers in front of call i."""
    tapped = []
    handle = mod.weight_fake_quant.register_forward_hook(lambda m, a, out: tapped.append(out.detach().clone()))
    calls = []
    for i, x in enumerate(inputs):
        rec = {}
        if load_bn_before is not None:
            load_bn_before(i, mod)
        if hasattr(mod, "bn"):
            for b in BN_BUFFERS:
                rec["bn_before." + b] = getattr(mod.bn, b).detach().clone()
        with torch.no_grad():
            rec["out"] = mod(x).detach().clone()
        rec["wq"] = tapped[-1]
        assert len(tapped) == i + 1, "the weight fake-quantizer is called once per forward"
        rec["scale"] = mod.weight_fake_quant.scale.detach().clone()
        rec["amax_history"] = mod.weight_fake_quant.amax_history.detach().clone()
        if hasattr(mod, "bn"):
            for b in BN_BUFFERS:
                rec["bn_after." + b] = getattr(mod.bn, b).detach().clone()
        calls.append(rec)
    handle.remove()
    return calls


class MiniCNN(nn.Module):
    def __init__(self):
        super().__init__()
        self.c1 = nn.Conv2d(3, 64, 3, padding=1, bias=False)
        self.b1 = nn.BatchNorm2d(64)
        self.r1 = nn.ReLU()
        self.c2 = nn.Conv2d(64, 64, 3, stride=2)
        self.fc = nn.Linear(64, 10)

    def forward(self, x):
        x = self.r1(self.b1(self.c1(x)))
        x = self.c2(x)
        return self.fc(x.amax((2, 3)))


CNN_ARGS = dict(activation="int8,qs=per_tensor_symmetric", weight="int8,qs=per_tensor_symmetric", quantize_forward="gemm", bf16=True,
                force_scale_power_of_two=True)
CNN_INPUT = (4, 3, 12, 10)


def build_cnn(impl, device=None):
    """MiniCNN with seeded parameters, conv + BN fused for QAT, then the implementation's quantize()."""
    from torch.ao.quantization import fuse_modules_qat
    m = seed_params_(MiniCNN(), 3000).train()
    fuse_modules_qat(m, [["c1", "b1"]], inplace=True)
    if device is not None:
        m.to(device)
    return impl.quantize(m, impl.make_args(**CNN_ARGS))


def cnn_batches():
    return [(rand_bf16(3200 + i, CNN_INPUT), torch.from_numpy(np.random.default_rng(3300 + i).integers(0, 10, CNN_INPUT[0]))) for i in range(3)]


def train_cnn(m, lr=0.05):
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    for x, t in cnn_batches():
        opt.zero_grad()
        nn.functional.cross_entropy(m(x.to(next(m.parameters()).device)).float(), t.to(next(m.parameters()).device)).backward()
        opt.step()
    return m


def freeze_for_eval(m):
    """BN frozen, observers disabled, eval mode: the state in which the checkpoint's logits were taken."""
    for mod in m.modules():
        if hasattr(mod, "freeze_bn_stats"):
            mod.freeze_bn_stats()
        if hasattr(mod, "observer_enabled") and hasattr(mod, "disable_observer"):
            mod.disable_observer()
    return m.eval()


# ---- the generator proper ------------------------------------------------------------------------------------------------------------
def _ref_impl():
    sys.path.insert(0, HERE)
    import torch.ao.nn.intrinsic as nni
    from _ref_import import load_reference
    ref = load_reference(with_quantize=True)
    # upstream's conv entries of DEFAULT_QAT_MODULE_MAPPINGS (quantization_mappings.py:16-25); the shim's dict holds nn.Linear only
    ref.quantize.DEFAULT_QAT_MODULE_MAPPINGS.update({
        nn.Conv2d: ref.nnqat.Conv2d, nn.Conv3d: ref.nnqat.Conv3d,
        nni.ConvBn1d: ref.nnqat.ConvBn1d, nni.ConvBn2d: ref.nnqat.ConvBn2d, nni.ConvBn3d: ref.nnqat.ConvBn3d,
    })

    def make_args(**kw):
        a = ref.training_args.add_qspec_args().parse_args([])
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    return Impl(ref.nnqat, ref.qconfig.get_qconfig, ref.quantize.quantize, make_args)


def gen_traces(impl, out):
    arrays, meta = {}, {}

    def put(key, calls, extra=None):
        for i, rec in enumerate(calls):
            for k, v in rec.items():
                arrays[f"{key}/call{i}/{k}"] = bits(v)
        meta[key] = {"calls": len(calls), "dtypes": {k: str(v.dtype).replace("torch.", "") for k, v in calls[0].items()}, **(extra or {})}

    for spec in SPECS:
        for name, (_, _, shape) in LAYERS.items():
            xs = activation_inputs(impl, spec, shape, 40 + len(name))
            for i, x in enumerate(xs):
                arrays[f"{spec}/{name}/x{i}"] = bits(x)
            put(f"{spec}/{name}", run_trace(build_layer(impl, spec, name), xs))
        xs = activation_inputs(impl, spec, CONVBN_INPUT, 77)
        for i, x in enumerate(xs):
            arrays[f"{spec}/convbn2d/x{i}"] = bits(x)
        for mode in CONVBN_MODES:
            m = build_convbn(impl, spec, mode)
            calls = run_trace(m, xs)
            extra = {"bn_training": bool(m.bn.training), "training": bool(m.training)}
            if mode == "train_frozen":
                f = m.to_float()
                arrays[f"{spec}/convbn2d/{mode}/to_float.weight"] = bits(f.weight)
                arrays[f"{spec}/convbn2d/{mode}/to_float.bias"] = bits(f.bias)
                extra["to_float"] = type(f).__name__
            put(f"{spec}/convbn2d/{mode}", calls, extra)
    np.savez_compressed(os.path.join(out, "conv_traces.npz"), **{k.replace("/", "__"): v for k, v in arrays.items()})
    with open(os.path.join(out, "conv_traces.json"), "w") as f:
        json.dump(meta, f, indent=1)


def gen_cnn(impl, out):
    m = build_cnn(impl)
    meta = {"modules": [(n, type(mod).__name__) for n, mod in m.named_modules()],
            "state_dict_keys": sorted(m.state_dict().keys())}
    train_cnn(m)
    sd = m.state_dict()
    meta["state_dict"] = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()}
    arrays = {"sd/" + k: bits(v) for k, v in sd.items()}
    freeze_for_eval(m)
    x = rand_bf16(3400, CNN_INPUT)
    with torch.no_grad():
        y = m(x)
    arrays["eval/x"] = bits(x)
    arrays["eval/logits"] = bits(y)
    meta["eval_dtype"] = str(y.dtype).replace("torch.", "")
    np.savez_compressed(os.path.join(out, "conv_cnn.npz"), **{k.replace("/", "__"): v for k, v in arrays.items()})
    with open(os.path.join(out, "conv_cnn.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    torch.manual_seed(0)
    ref_impl = _ref_impl()
    gen_traces(ref_impl, HERE)
    gen_cnn(ref_impl, HERE)
    print("wrote conv_traces.{npz,json}, conv_cnn.{npz,json}")
