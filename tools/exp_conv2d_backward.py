"""bf16 NHWC Conv2d backward, both routes in one process on one box: the in-tree implicit-GEMM kernels (qt_conv2d_dgrad_bf16 /
qt_conv2d_wgrad_bf16, csrc/qt_conv_backward.hip) against what the library runs for the same product -- aten.convolution_backward with
the single-product output mask on the same saved tensors (channels_last gradient and input, the weight as the module holds it) -- on
ResNet-50's body layers at batch 32, the shape list of profiles/conv2d_routes.txt.  The route's own layout copy (the [Cout][kh][kw][Cin]
copy of the weight the input gradient reads; the forward makes it and the Function keeps it, so a training step pays it once) is timed
beside the kernels and counted against the input gradient.  Operands rotate over a pool larger than the Infinity Cache.  Timing: warm-up,
then REPEATS timed runs of ITERS launches each between two events; the median of the repeats with min / max beside it; "spread" is
(max - min) / median of the LIBRARY's repeats, the run-to-run noise a product must beat to go in-tree under QT_CONV_GEMM=auto.
The table this prints is committed as profiles/conv2d_bwd_routes.txt and decides conv_route._auto_takes_dgrad / _auto_takes_wgrad.

    timeout -k 10 900 python tools/exp_conv2d_backward.py [--iters 20] [--repeats 7] [--shapes 3x3|1x1|all]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
from quantized_training import _native, conv_route  # noqa: E402

DEV = "cuda:0"
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
    per_set = BATCH * hw * hw * (2 * cin + 2 * cout) * 2 + 2 * cout * k * k * cin * 2
    pool = int(max(2, min(48, POOL_BYTES // per_set + 1)))
    g = torch.Generator(device=DEV).manual_seed(0)
    cl = torch.channels_last
    xs = [torch.randn((BATCH, cin, hw, hw), generator=g, device=DEV).bfloat16().contiguous(memory_format=cl) for _ in range(pool)]
    gys = [(torch.randn((BATCH, cout, hw, hw), generator=g, device=DEV) * 0.1).bfloat16().contiguous(memory_format=cl) for _ in range(pool)]
    wqs = [(torch.randn((cout, cin, k, k), generator=g, device=DEV) * 0.05).bfloat16() for _ in range(pool)]     # as the module holds it
    wks = [w.contiguous(memory_format=cl) for w in wqs]                                                         # [Cout][kh][kw][Cin]
    gxs = [torch.empty_like(x) for x in xs]
    gws = [torch.empty((cout, k, k, cin), dtype=torch.bfloat16, device=DEV) for _ in range(pool)]
    ints = (BATCH, hw, hw, cin, cout, k, k, 1, 1, pad, pad, 1, 1)
    d, gp = conv_route.backward_plan(*ints)
    ws = torch.empty((max(gp.ws_bytes // 4, 4),), dtype=torch.float32, device=DEV)
    tickets = torch.zeros((max(gp.n_tickets, 4),), dtype=torch.int32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.note_device(0)

    def dgrad(i):
        j = i % pool
        rc = L.qt_conv2d_dgrad_bf16(gys[j].data_ptr(), wks[j].data_ptr(), gxs[j].data_ptr(), *ints, stream)
        assert rc == 0, rc

    def wgrad(i):
        j = i % pool
        rc = L.qt_conv2d_wgrad_bf16(gys[j].data_ptr(), xs[j].data_ptr(), gws[j].data_ptr(), *ints, ws.data_ptr(), ws.numel() * 4, tickets.data_ptr(),
                                    tickets.numel(), stream)
        assert rc == 0, rc

    def lib(mask):
        def run(i):
            j = i % pool
            return torch.ops.aten.convolution_backward(gys[j], xs[j], wqs[j], None, [1, 1], [pad, pad], [1, 1], False, [0, 0], 1, mask)
        return run

    def weight_copy(i):
        return wqs[i % pool].contiguous(memory_format=cl)

    dgrad(0)
    wgrad(0)
    rx, rw = lib([True, False, False])(0)[0], lib([False, True, False])(0)[1]
    err_d = (gxs[0].float() - rx.float()).abs().max().item() / rx.float().abs().max().item()
    err_w = (gws[0].permute(0, 3, 1, 2).float() - rw.float()).abs().max().item() / rw.float().abs().max().item()
    t_d, t_w, t_c = timed(dgrad, iters, repeats), timed(wgrad, iters, repeats), timed(weight_copy, iters, repeats)
    l_d, l_w = timed(lib([True, False, False]), iters, repeats), timed(lib([False, True, False]), iters, repeats)
    sp_d, sp_w = (l_d[2] - l_d[1]) / l_d[0], (l_w[2] - l_w[1]) / l_w[0]
    r_d, r_w = l_d[0] / (t_d[0] + t_c[0]), l_w[0] / t_w[0]
    auto_d = conv_route._auto_takes_dgrad(BATCH * hw * hw, cin, d.k_tiles)
    auto_w = conv_route._auto_takes_wgrad(BATCH * hw * hw, cout, k * k * cin, gp.ksplit)
    print(f"{BATCH}x{cin}x{hw}x{hw} -> {cout} {k}x{k} "
          f"| dgrad tile {d.tile_m}x{d.tile_n} grid {d.tiles_m}x{d.tiles_n} k tiles {d.k_tiles:3d}: in-tree {t_d[0]:7.1f} us [{t_d[1]:7.1f} {t_d[2]:7.1f}] "
          f"+ weight copy {t_c[0]:5.1f} us, library {l_d[0]:7.1f} us [{l_d[1]:7.1f} {l_d[2]:7.1f}] spread {100 * sp_d:4.1f} %, "
          f"library / (in-tree + copy) {r_d:5.2f}, auto -> {'in-tree' if auto_d else 'library'}, max rel diff {err_d:.1e} "
          f"| wgrad tile {gp.tile_m}x{gp.tile_n} grid {gp.tiles_m}x{gp.tiles_n} k tiles {gp.k_tiles:4d} split {gp.ksplit:2d}: in-tree {t_w[0]:7.1f} us "
          f"[{t_w[1]:7.1f} {t_w[2]:7.1f}], library {l_w[0]:7.1f} us [{l_w[1]:7.1f} {l_w[2]:7.1f}] spread {100 * sp_w:4.1f} %, library / in-tree {r_w:5.2f}, "
          f"auto -> {'in-tree' if auto_w else 'library'}, max rel diff {err_w:.1e} | pool {pool}", flush=True)
    return max(sp_d, sp_w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default="all", choices=["all", "3x3", "1x1"])
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {args.repeats} repeats of {args.iters} launches [min max]; "
          f"library = aten.convolution_backward with the single-product output mask, bf16 channels_last gradient and input", flush=True)
    shapes = (SHAPES_3X3 if args.shapes in ("all", "3x3") else []) + (SHAPES_1X1 if args.shapes in ("all", "1x1") else [])
    spread = max(bench(*s, args.iters, args.repeats) for s in shapes)
    print(f"# largest run-to-run spread (max - min) / median of the library's repeats in this table: {100 * spread:.1f} %")


if __name__ == "__main__":
    main()
