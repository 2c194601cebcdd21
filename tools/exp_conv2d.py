"""bf16 NHWC Conv2d forward, both routes in one process on one box: the in-tree implicit-GEMM kernel (qt_conv2d_bf16, csrc/qt_conv.hip)
against the library's convolution (torch.nn.functional.conv2d on channels_last operands -> MIOpen), on ResNet-50's body layers at batch 32.
Operands rotate over a pool larger than the Infinity Cache (as tools/exp_linear_fq8.py does), so neither route is timed on cache-resident
activations.  Timing: warm-up, then REPEATS timed runs of ITERS launches each between two events; the median of the repeats with min / max
beside it.  The table this prints is committed as profiles/conv2d_routes.txt and decides the QT_CONV_GEMM=auto rule (conv_route._auto_takes).

    timeout -k 10 900 python tools/exp_conv2d.py [--iters 20] [--repeats 7] [--shapes 3x3|1x1|all]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
from quantized_training import _native, conv_route  # noqa: E402

DEV = "cuda:0"
PEAK_TFLOPS = 2500.0          # dense bf16 peak the project quotes
POOL_BYTES = 320e6            # > the 256 MB Infinity Cache

# (H = W, Cin, Cout, k): ResNet-50 body layers, batch 32, stride 1, padding k // 2
SHAPES_3X3 = [(56, 64, 64, 3), (28, 128, 128, 3), (14, 256, 256, 3), (7, 512, 512, 3)]
SHAPES_1X1 = [(56, 64, 64, 1), (56, 64, 256, 1), (56, 256, 64, 1), (28, 128, 512, 1), (28, 512, 128, 1), (14, 256, 1024, 1), (14, 1024, 256, 1),
              (7, 512, 2048, 1), (7, 2048, 512, 1)]
BATCH = 32


def timed(fn, iters, repeats):
    for i in range(5):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for r in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(iters):
            fn(r * iters + i)
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def bench(hw, cin, cout, k, iters, repeats):
    L = _native.lib()
    pad = k // 2
    per_set = BATCH * hw * hw * (cin + cout) * 2 + cout * k * k * cin * 2
    pool = int(max(2, min(64, POOL_BYTES // per_set + 1)))
    g = torch.Generator(device=DEV).manual_seed(0)
    xs = [torch.randn((BATCH, cin, hw, hw), generator=g, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last) for _ in range(pool)]
    ws = [(torch.randn((cout, cin, k, k), generator=g, device=DEV) * 0.05).bfloat16().contiguous(memory_format=torch.channels_last)
          for _ in range(pool)]
    ys = [torch.empty((BATCH, cout, hw, hw), dtype=torch.bfloat16, device=DEV, memory_format=torch.channels_last) for _ in range(pool)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.note_device(0)

    def in_tree(i):
        j = i % pool
        rc = L.qt_conv2d_bf16(xs[j].data_ptr(), ws[j].data_ptr(), None, ys[j].data_ptr(), BATCH, hw, hw, cin, cout, k, k, 1, 1, pad, pad, 1, 1, stream)
        assert rc == 0, rc

    def library(i):
        j = i % pool
        return F.conv2d(xs[j], ws[j], None, 1, pad, 1, 1)

    def weight_copy(i):
        return ws[i % pool].permute(0, 2, 3, 1).clone()              # the per-forward [Cout][kh][kw][Cin] copy of the route

    in_tree(0)
    ref = library(0)
    err = (ys[0].float() - ref.float()).abs().max().item() / ref.float().abs().max().item()
    tile = [ctypes.c_int(0) for _ in range(5)]
    L.qt_conv2d_plan(BATCH, hw, hw, cin, cout, k, k, 1, 1, pad, pad, 1, 1, *[ctypes.byref(t) for t in tile])
    t_i, t_l, t_w = timed(in_tree, iters, repeats), timed(library, iters, repeats), timed(weight_copy, iters, repeats)
    flops = 2.0 * BATCH * hw * hw * cout * cin * k * k
    tf_i, tf_l = flops / t_i[0] / 1e6, flops / t_l[0] / 1e6
    print(f"{BATCH}x{cin}x{hw}x{hw} -> {cout} {k}x{k} | tile {tile[0].value}x{tile[1].value} grid {tile[2].value}x{tile[3].value} k tiles {tile[4].value:3d} "
          f"| in-tree {t_i[0]:7.1f} us [{t_i[1]:7.1f} {t_i[2]:7.1f}] {tf_i:6.0f} TFLOP/s ({100 * tf_i / PEAK_TFLOPS:4.1f} % of {PEAK_TFLOPS:.0f}) "
          f"| library {t_l[0]:7.1f} us [{t_l[1]:7.1f} {t_l[2]:7.1f}] {tf_l:6.0f} TFLOP/s | library / in-tree {t_l[0] / t_i[0]:5.2f} "
          f"| per k tile {t_i[0] / tile[4].value:6.2f} us | weight copy {t_w[0]:5.1f} us: library / (in-tree + copy) {t_l[0] / (t_i[0] + t_w[0]):5.2f} "
          f"| auto -> {'in-tree' if conv_route._auto_takes(BATCH * hw * hw, tile[4].value) else 'library'} | pool {pool} | max rel diff {err:.1e}", flush=True)
    return t_i[0] + t_w[0], t_l[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default="all", choices=["all", "3x3", "1x1"])
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {args.repeats} repeats of {args.iters} launches [min max]; "
          f"library = F.conv2d, bf16 channels_last operands", flush=True)
    shapes = (SHAPES_3X3 if args.shapes in ("all", "3x3") else []) + (SHAPES_1X1 if args.shapes in ("all", "1x1") else [])
    wins = 0
    for s in shapes:
        t_i, t_l = bench(*s, args.iters, args.repeats)
        wins += t_i <= t_l
    print(f"# in-tree + weight copy at least as fast as the library on {wins} of {len(shapes)} shapes")


if __name__ == "__main__":
    main()
