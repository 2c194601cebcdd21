"""conv2d_mx on integer and codebook operands, both routes in one process on one box: the operator on the integer matrix cores (qt_mxi_pack +
qt_conv2d_mxi, csrc/qt_mxi_conv.hip, through quantized_training/mx_conv.py) against the composite it replaces (QT_MX_GEMM=0: codebook
gather, both operands times their expanded block scales, then the library's convolution), on ResNet-50's body layers at batch 32 -- the
shapes of profiles/conv2d_mx.txt -- in bf16 and fp32, with `int6,bs=64,scale=fp8_e5m3` activations and nf4_6 / int6 weights.

The activation is a channels_last tensor quantized by quantize_mx along the channel axis; its pack (qt_mxi_pack through the strides) runs
inside the timed call, the weight operand is packed once and cached, as in a converted model.  Operands rotate over a pool larger than
the Infinity Cache.  Timing: warm-up, then REPEATS rounds; a round times ITERS calls of each route between two events, the routes
alternating inside the round; the median of the rounds with the spread (max - min) / median beside it.  A row clears the bar when the
native median beats the composite's by more than the composite's spread.  The table this prints is committed as profiles/conv2d_mxi.txt
and decides which shape classes mx_conv._int_conv_route_takes lists (the tool switches the rule off so that every layer is timed natively).

    timeout -k 10 900 python tools/exp_conv2d_mxi.py [--iters 200] [--repeats 7] [--weights nf4_6,int6] [--dtypes bf16,fp32]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
from quantized_training import mx_conv, mx_gemm  # noqa: E402
from quantized_training.fake_quantize import get_quantization_map  # noqa: E402
from quantized_training.quantizer.quantizer import get_quant_min_max  # noqa: E402

DEV = "cuda:0"
POOL_BYTES = 320e6            # > the 256 MB Infinity Cache
BATCH = 32
BS = 64
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
# (H = W, Cin, Cout, k): ResNet-50 body layers, stride 1, padding k // 2
SHAPES = [(56, 64, 64, 3), (28, 128, 128, 3), (14, 256, 256, 3), (7, 512, 512, 3), (56, 64, 64, 1), (56, 64, 256, 1), (56, 256, 64, 1),
          (28, 128, 512, 1), (28, 512, 128, 1), (14, 256, 1024, 1), (14, 1024, 256, 1), (7, 512, 2048, 1), (7, 2048, 512, 1)]


def quantized(x, fmt):
    """(values or indices, block scales rounded to fp8_e5m3, codebook or None) through quantize_mx along the channel axis."""
    qmap, code = get_quantization_map(fmt, DEV), None
    if isinstance(qmap, tuple):
        qmap, code = qmap[0], qmap[1].to(x.dtype)
    s, q = torch.ops.quantized_ops.quantize_mx(x, qmap, [1], BS, float(get_quant_min_max(fmt)[1]), False,
                                               get_quantization_map("fp8_e5m3", DEV), None)
    return q, s, code


def rounds(fns, iters, repeats):
    """{name: (median, spread)} in us per call; the routes alternate inside every round."""
    for fn in fns.values():
        for i in range(5):
            fn(i)
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for r in range(repeats):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(iters):
                fn(r * iters + i)
            e.record()
            torch.cuda.synchronize()
            out[name].append(s.elapsed_time(e) * 1e3 / iters)
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in out.items()}


def bench(dname, wfmt, hw, cin, cout, k, iters, repeats):
    dtype, pad = DTYPES[dname], k // 2
    esz = 2 if dtype == torch.bfloat16 else 4
    per_set = BATCH * hw * hw * (cin * (esz + 1) + cout * esz) + cout * k * k * cin * (esz + 1)
    pool = int(max(2, min(32, POOL_BYTES // per_set + 1)))
    g = torch.Generator(device=DEV).manual_seed(0)
    conv = torch.ops.quantized_ops.conv2d_mx
    acts, weights = [], []
    for _ in range(pool):
        x = (torch.randn((BATCH, cin, hw, hw), generator=g, device=DEV) * 2).to(dtype).contiguous(memory_format=torch.channels_last)
        w = (torch.randn((cout, cin, k, k), generator=g, device=DEV) * 0.05).to(dtype)
        acts.append(quantized(x, "int6"))
        weights.append(quantized(w, wfmt))

    def call(i):
        j = i % pool
        (x, xs, xc), (w, ws, wc) = acts[j], weights[j]
        return conv(x, w, None, [1, 1], [pad, pad], [1, 1], 1, input_scale=xs, weight_scale=ws, block_size=BS, input_code=xc, weight_code=wc)

    def composite(i):
        os.environ["QT_MX_GEMM"] = "0"
        try:
            return call(i)
        finally:
            os.environ["QT_MX_GEMM"] = "1"

    mx_gemm.STATS.reset()
    y, ref = call(0), composite(0)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0), "the native route declined this shape"
    err = (y.float() - ref.float()).abs().max().item() / ref.float().abs().max().item()
    t = rounds({"native": call, "composite": composite}, iters, repeats)
    (tn, sn), (tc, sc) = t["native"], t["composite"]
    m, kk = BATCH * hw * hw, k * k * cin
    cleared = tn < tc * (1.0 - sc)
    print(f"{dname} int6 x {wfmt} {BATCH}x{cin}x{hw}x{hw} -> {cout} {k}x{k} | m {m} cout {cout} k {kk} | native + pack {tn:7.1f} us (spread {100 * sn:4.1f} %) "
          f"| composite {tc:7.1f} us (spread {100 * sc:4.1f} %) | composite / native {tc / tn:5.2f} | bar {'cleared' if cleared else 'missed'} "
          f"| rule -> {'native' if mx_conv._int_conv_route_takes(m, cout, kk, k * k, dtype) else 'composite'} | pool {pool} | max rel diff {err:.1e}", flush=True)
    return cleared


def main():
    mx_conv._APPLY_INT_CONV_RULE = False                            # time every layer on both routes, the declined classes included
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--weights", default="nf4_6,int6")
    ap.add_argument("--dtypes", default="bf16,fp32")
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; the operator conv2d_mx, int6 activations, block size {BS}, fp8_e5m3 scales; "
          f"median of {args.repeats} rounds of {args.iters} calls per route, routes alternating (spread = (max - min) / median); "
          f"bar: native < composite * (1 - composite's spread)", flush=True)
    for dname in args.dtypes.split(","):
        for wfmt in args.weights.split(","):
            n = sum(bench(dname, wfmt, *s, args.iters, args.repeats) for s in SHAPES)
            print(f"# {dname}, int6 x {wfmt}: the bar is cleared on {n} of {len(SHAPES)} shapes", flush=True)


if __name__ == "__main__":
    main()
