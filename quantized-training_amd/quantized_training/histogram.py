"""Exponent histograms (`record_histogram`, upstream fake_quantize.py:348-350) and the plots made from them (upstream histogram.py).

Recording.  The reference runs, per quantizer call,

    exp = torch.floor(torch.log2(torch.abs(X.detach().float())))
    self.histogram += torch.histc(exp, 254, min=-126, max=127)

On a bf16 / fp16 device tensor this is one launch of qt_exp_histogram_* instead (csrc/qt_histogram.hip): for such an element,
converted exactly to fp32, the bin is the fp32 exponent field E = (bits >> 23) & 0xFF -- 1 <= E <= 254 counts into bin E - 1, zeros,
fp32-subnormal magnitudes, inf and NaN count nowhere, exactly as histc leaves them out (enumerated over all 65 536 patterns of both
types, tests/test_histogram_cpu.py).  fp32 inputs are NOT taken: for most of the values one ulp below a power of two
floor(log2f(x)) rounds up into the next bin, which depends on the library's log2f, so they keep the composite.  Neither are CPU
tensors, a histogram buffer that is not contiguous fp32[254] on the tensor's device (`model.to(torch.bfloat16)` makes it bf16),
overlapping or non-dense views, 2^32 elements or more, or anything at all with QT_HISTOGRAM=0.  A histogram does not depend on the
order of the elements, so a dense view in any dimension order is read as its storage lies.

STATS counts the calls by route: histogram_native (the stand-alone launch), histogram_fused (taken inside the fake-quant pass,
qt_fake_quant_hist_bf16), histogram_composite (the two lines above).
"""
import ctypes
import os
import re
from collections import defaultdict

import torch

from . import _native, switches

STATS = {"histogram_native": 0, "histogram_fused": 0, "histogram_composite": 0}
BINS = 254
_KERNEL_DTYPES = (torch.bfloat16, torch.float16)


def reset_stats():
    for k in STATS:
        STATS[k] = 0


def _dense(t):
    """Non-overlapping and dense in some dimension order: sorted by stride, every stride is the product of the sizes below it."""
    if t.is_contiguous():
        return True
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda p: p[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def eligible(X, hist):
    """The rule of the module docstring: what the kernel takes."""
    return (switches.on("QT_HISTOGRAM") and X.device.type == "cuda" and X.dtype in _KERNEL_DTYPES
            and hist.device == X.device and hist.dtype == torch.float32 and hist.numel() == BINS and hist.is_contiguous()
            and X.numel() < (1 << 32) and _dense(X))


def scratch(device):
    """(counts address, ticket address) of the zero-kept scratch for the launch about to be issued on `device`'s current stream."""
    from . import fused
    _, words = fused.splitk_scratch("hist", 0, 257, device)
    return words.data_ptr(), words.data_ptr() + 256 * 4


def _stream_ptr(t):
    _native.note_device(t.device.index)
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def composite(X, hist):
    """The reference's two lines, verbatim."""
    exp = torch.floor(torch.log2(torch.abs(X.detach().float())))
    hist += torch.histc(exp, 254, min=-126, max=127)
    STATS["histogram_composite"] += 1


def exp_histogram_or_none(X, hist):
    """hist += the exponent histogram of X in one launch; `hist` when the kernel took the call, else None (nothing done)."""
    if not eligible(X, hist):
        return None
    n = X.numel()
    if n:
        L = _native.lib()
        counts, ticket = scratch(X.device)
        fn = L.qt_exp_histogram_bf16 if X.dtype == torch.bfloat16 else L.qt_exp_histogram_f16
        _native.check(fn(X.data_ptr(), n, hist.data_ptr(), counts, ticket, _stream_ptr(X)), "qt_exp_histogram")
    STATS["histogram_native"] += 1
    return hist


def record(X, hist):
    """One record_histogram step on `hist`: the kernel where it applies, else the composite."""
    if exp_histogram_or_none(X, hist) is None:
        composite(X, hist)


def fused_state(X, hist):
    """(hist, counts address, ticket address) for qt_fake_quant_hist_bf16 when the fake-quant pass over the contiguous bf16 tensor X
    may take the histogram on the way, else None."""
    if X.dtype != torch.bfloat16 or not X.is_contiguous() or X.numel() == 0 or not eligible(X, hist):
        return None
    return (hist,) + scratch(X.device)


# ---- the plots (upstream histogram.py) ---------------------------------------------------------------------------------------
_GROUP = re.compile(r"(.*?\.\d+)\.(.*?)?(?=\.activation_pre_process\.\d+)")
_HOOK = re.compile(r"\.activation_pre_process\.\d+")


def get_grouped_histogram(model):
    """{group: [(layer name, histogram as a numpy array), ...]} over the model's fake-quantizers.  A name like
    `encoder.layer.3.attention.query.activation_pre_process.0` goes to group `encoder.layer.3` as `attention.query`; a name without a
    numbered block in front of `.activation_pre_process.N` is its own group and layer name, with that suffix removed."""
    from torch.ao.quantization import FakeQuantizeBase
    groups = defaultdict(list)
    for name, module in model.named_modules():
        if not isinstance(module, FakeQuantizeBase):
            continue
        m = _GROUP.search(name)
        if m:
            group, layer = m.group(1), m.group(2)
        else:
            group = layer = _HOOK.sub("", name)
        groups[group].append((layer, module.histogram.float().cpu().numpy()))
    return groups


def _pyplot():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    return plt


def plot_histogram(model, output_dir):
    """One `<group>.png` per group of get_grouped_histogram: every layer's normalised exponent histogram as a smoothed curve over the
    group's occupied exponents (from the 0.5 % quantile of the group's sum up to its highest occupied bin)."""
    import numpy as np
    from scipy.interpolate import make_interp_spline
    plt = _pyplot()
    for group, layers in get_grouped_histogram(model).items():
        total = np.sum(np.stack([h for _, h in layers]), axis=0)
        occupied = np.flatnonzero(total)
        if occupied.size == 0:
            continue                                                    # nothing recorded in this group
        lo = max(int(occupied.min()), int(np.searchsorted(np.cumsum(total) / total.sum(), 0.005)))
        hi = int(occupied.max())
        exponents = np.arange(lo, hi + 1) - 126
        plt.figure(figsize=(10, 6))
        for layer, h in layers:
            share = (h / h.sum())[lo:hi + 1] if h.sum() else np.zeros(hi + 1 - lo)
            if exponents.size >= 4:                                     # a cubic spline needs four points
                xs = np.linspace(exponents.min(), exponents.max(), 500)
                plt.plot(xs, make_interp_spline(exponents, share)(xs), label=layer)
            else:
                plt.plot(exponents, share, label=layer)
        plt.xlabel("Exponent Value")
        plt.ylabel("Frequency")
        plt.title(f"{group} Histogram")
        plt.legend(loc="upper left", bbox_to_anchor=(1, 1), ncol=1)
        plt.subplots_adjust(right=0.75)
        plt.savefig(os.path.join(output_dir, f"{group}.png"))
        plt.close()


def plot_layer_range(model, output_dir):
    """`layer_distribution.png`: one horizontal bar per layer name (summed over the groups) from its lowest to its highest occupied
    exponent, the low end clipped at the 0.5 % quantile of the whole model's histogram."""
    import numpy as np
    plt = _pyplot()
    per_layer = {}
    for layers in get_grouped_histogram(model).values():
        for layer, h in layers:
            layer = layer.replace("activation_pre_process.", "")
            per_layer[layer] = per_layer.get(layer, 0) + h
    per_layer = {k: h for k, h in per_layer.items() if np.any(h)}
    if not per_layer:
        return
    total = np.sum(np.stack(list(per_layer.values())), axis=0)
    floor = int(np.searchsorted(np.cumsum(total) / total.sum(), 0.005)) - 126
    ranges = {}
    for layer, h in per_layer.items():
        occupied = np.flatnonzero(h) - 126
        ranges[layer] = (max(floor, int(occupied.min())), int(occupied.max()))
    fig, ax = plt.subplots(figsize=(8, 6))
    rows = list(range(len(ranges)))
    ax.barh(rows, [hi - lo for lo, hi in ranges.values()], left=[lo for lo, _ in ranges.values()], height=1, color="tab:blue",
            edgecolor="black", linewidth=0.5)
    ax.set_yticks(rows)
    ax.set_yticklabels(list(ranges))
    ax.set_ylim(-0.5, len(rows) - 0.5)
    for side in ("top", "right", "left"):
        ax.spines[side].set_visible(False)
    ax.axvline(x=0, color="black", linewidth=0.75)
    ax.tick_params(axis="y", which="both", left=False)
    ax.set_xlabel("Exponent Value", fontsize=16)
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, "layer_distribution.png"), dpi=300)
    plt.close()
