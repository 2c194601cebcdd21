"""conv2d_mx, both routes in one process on one box: the operator on the block-scaled matrix instruction (qt_conv2d_mx, csrc/qt_mx_conv.hip,
through quantized_training/mx_conv.py) against the composite it replaces (QT_MX_GEMM=0: both operands times their expanded block scales,
then the library's convolution), on ResNet-50's body layers at batch 32 -- the shapes of profiles/conv2d_routes.txt.

The activation is what a layer behind an in-tree convolution receives: a channels_last bf16 tensor quantized by quantize_mx along the
channel axis, which leaves the packed NHWC operand on its result ("native"); "native + pack" is the same call after that operand has been
dropped, so that qt_mx_pack runs inside the timed call.  The weight operand is packed once and cached, as in a converted model.  Operands
rotate over a pool larger than the Infinity Cache.  Timing: warm-up, then REPEATS rounds; a round times ITERS calls of each route between
two events, the routes alternating inside the round; the median of the rounds with the spread (max - min) / median beside it.  The table
this prints is committed as profiles/conv2d_mx.txt and decides which shape class mx_conv declines (mx_conv._pack_route_takes; the tool
switches the rule off so that every layer is timed on every route).

    timeout -k 10 900 python tools/exp_conv2d_mx.py [--iters 20] [--repeats 7] [--formats fp8_e4m3,fp4_e2m1]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
from quantized_training import mx_conv, mx_gemm, mx_operand  # noqa: E402
from quantized_training.fake_quantize import get_quantization_map  # noqa: E402
from quantized_training.quantizer.quantizer import get_quant_min_max  # noqa: E402

DEV = "cuda:0"
POOL_BYTES = 320e6            # > the 256 MB Infinity Cache
BATCH = 32
# (H = W, Cin, Cout, k): ResNet-50 body layers, stride 1, padding k // 2
SHAPES = [(56, 64, 64, 3), (28, 128, 128, 3), (14, 256, 256, 3), (7, 512, 512, 3), (56, 64, 64, 1), (56, 64, 256, 1), (56, 256, 64, 1),
          (28, 128, 512, 1), (28, 512, 128, 1), (14, 256, 1024, 1), (14, 1024, 256, 1), (7, 512, 2048, 1), (7, 2048, 512, 1)]


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


def bench(fmt, hw, cin, cout, k, iters, repeats):
    pad = k // 2
    qmap, qmax = get_quantization_map(fmt, DEV), float(get_quant_min_max(fmt)[1])
    per_set = BATCH * hw * hw * (cin * 3 + cout * 2) + cout * k * k * cin * 3
    pool = int(max(2, min(48, POOL_BYTES // per_set + 1)))
    g = torch.Generator(device=DEV).manual_seed(0)
    conv = torch.ops.quantized_ops.conv2d_mx
    acts, stripped, weights = [], [], []
    for _ in range(pool):
        x = (torch.randn((BATCH, cin, hw, hw), generator=g, device=DEV) * 2).bfloat16().contiguous(memory_format=torch.channels_last)
        w = (torch.randn((cout, cin, k, k), generator=g, device=DEV) * 0.05).bfloat16()
        xs, xq = torch.ops.quantized_ops.quantize_mx(x, qmap, [1], 32, qmax, True, None, None)
        ws, wq = torch.ops.quantized_ops.quantize_mx(w, qmap, [1], 32, qmax, True, None, None)
        assert mx_operand.operand_record(xq, mx_operand.NHWC) is not None
        bare = xq.detach()                                            # the same memory without the packed operand
        mx_operand.set_format(bare, mx_operand.format_of(xq))
        acts.append((xq, xs)); stripped.append((bare, xs)); weights.append((wq, ws))

    def call(src, i):
        j = i % pool
        return conv(src[j][0], weights[j][0], None, [1, 1], [pad, pad], [1, 1], 1, input_scale=src[j][1], weight_scale=weights[j][1], block_size=32)

    def native(i):
        return call(acts, i)

    def native_pack(i):
        return call(stripped, i)

    def composite(i):
        os.environ["QT_MX_GEMM"] = "0"
        try:
            return call(acts, i)
        finally:
            os.environ["QT_MX_GEMM"] = "1"

    mx_gemm.STATS.reset()
    y, ref = native(0), composite(0)
    native_pack(0)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (2, 0), "the native route declined this shape"
    err = (y.float() - ref.float()).abs().max().item() / ref.float().abs().max().item()
    t = rounds({"native": native, "composite": composite, "native + pack": native_pack}, iters, repeats)
    (tn, sn), (tc, sc), (tp, sp) = t["native"], t["composite"], t["native + pack"]
    flops = 2.0 * BATCH * hw * hw * cout * cin * k * k
    print(f"{fmt} {BATCH}x{cin}x{hw}x{hw} -> {cout} {k}x{k} | native {tn:7.1f} us (spread {100 * sn:4.1f} %) {flops / tn / 1e6:6.0f} TFLOP/s "
          f"| composite {tc:7.1f} us (spread {100 * sc:4.1f} %) | composite / native {tc / tn:5.2f} "
          f"| native + pack {tp:7.1f} us (spread {100 * sp:4.1f} %): composite / (native + pack) {tc / tp:5.2f} | rule without a packed operand -> "
          f"{'native' if mx_conv._pack_route_takes(k * k * cin) else 'composite'} | pool {pool} | max rel diff {err:.1e}", flush=True)
    return tn, tc, sc, tp


def main():
    mx_conv._APPLY_PACK_RULE = False                                # time every layer on every route, the declined class included
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--formats", default="fp8_e4m3,fp4_e2m1")
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; the operator conv2d_mx, bf16, block size 32; median of {args.repeats} rounds "
          f"of {args.iters} calls per route, routes alternating (spread = (max - min) / median)", flush=True)
    for fmt in args.formats.split(","):
        slower = []
        for s in SHAPES:
            tn, tc, sc, tp = bench(fmt, *s, args.iters, args.repeats)
            if tn > tc * (1.0 + sc):
                slower.append(s)
        print(f"# {fmt}: native slower than the composite by more than the composite's spread on {len(slower)} of {len(SHAPES)} shapes: {slower}", flush=True)


if __name__ == "__main__":
    main()
