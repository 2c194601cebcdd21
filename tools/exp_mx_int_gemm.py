"""linear_mx / matmul_mx on integer operands, both routes in one process on one box: the integer block-scaled GEMM (qt_mxi_pack +
qt_mxi_gemm, csrc/qt_mxi_gemm.hip, through quantized_training/mx_gemm.py) against the composite it replaces (QT_MX_GEMM=0: both operands
times their expanded block scales, then the library's GEMM).

Rows: LLaMA-2-7B's projections at 1024 tokens in bf16 and fp32 with `int6,bs=64,scale=fp8_e5m3` and `int8,bs=32`; Q . K^T and P . V of
[1, 32, 1024, 128] with `int6,bs=64` along ax = -1 / -2; small Linears from the size of the outlier showcase (tests/golden/outlier.json)
up to 256 x 256 x 256, and one in between.
The operands are what quantize_mx leaves; the weight's operand is packed once and cached, as in a converted model; the activation pack
runs inside the timed call.  "kernel" is qt_mxi_gemm alone on operands packed beforehand.  Operands rotate over a pool larger than the
Infinity Cache where memory allows.  Timing: warm-up, then REPEATS rounds; a round times ITERS calls of each route between two events,
the routes alternating inside the round; the median of the rounds with the spread (max - min) / median beside it.  A last block times
the kernel alone at 1024 x 4096 x 4096 for the three block sizes: the matrix instructions of bs = 64 and bs = 128 are the same, the
conversions, scale products and fmas beside them halve, so the ratio of the two says which pipe bounds the kernel.
The table this prints is committed as profiles/mx_int_gemm.txt and decides mx_gemm._int_route_takes (the tool switches the rule off so
that every row is timed on every route).

    timeout -k 10 900 python tools/exp_mx_int_gemm.py [--iters 10] [--repeats 5]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
from quantized_training import mx_gemm  # noqa: E402
from quantized_training.fake_quantize import get_quantization_map  # noqa: E402
from quantized_training.quantizer.quantizer import get_quant_min_max  # noqa: E402

DEV = "cuda:0"
POOL_BYTES = 320e6            # > the 256 MB Infinity Cache
CONFIGS = {"int6,bs=64,scale=fp8_e5m3": ("int6", 64, "fp8_e5m3"), "int8,bs=32": ("int8", 32, None), "int6,bs=64": ("int6", 64, None)}
LINEARS = [(1024, 4096, 4096), (1024, 11008, 4096), (1024, 4096, 11008)]          # M (tokens), N, K
SMALL = [(16, 128, 64), (16, 64, 128), (152, 72, 192), (256, 256, 256)]
MID = [(512, 1024, 1024)]
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def rounds(fns, iters, repeats):
    """{name: (median, spread)} in us per call; the routes alternate inside every round."""
    for fn in fns.values():
        for i in range(3):
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


def quantized(x, fmt, bs, axis, scale_fmt):
    smap = get_quantization_map(scale_fmt, DEV) if scale_fmt else None
    s, q = torch.ops.quantized_ops.quantize_mx(x, get_quantization_map(fmt, DEV), [axis], bs, float(get_quant_min_max(fmt)[1]), False, smap, None)
    return q, s


def composite_of(fn):
    def run(i):
        os.environ["QT_MX_GEMM"] = "0"
        try:
            return fn(i)
        finally:
            os.environ["QT_MX_GEMM"] = "1"
    return run


def report(label, flops, native, composite, kernel, iters, repeats, pool, rule):
    mx_gemm.STATS.reset()
    y, ref = native(0), composite(0)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0), "the native route declined this row"
    err = (y.float() - ref.float()).abs().max().item() / ref.float().abs().max().item()
    t = rounds({"native": native, "composite": composite, "kernel": kernel}, iters, repeats)
    (tn, sn), (tc, sc), (tk, sk) = t["native"], t["composite"], t["kernel"]
    wins = tn < tc * (1.0 - sc)
    print(f"{label} | native {tn:8.1f} us (spread {100 * sn:4.1f} %) | composite {tc:8.1f} us (spread {100 * sc:4.1f} %) | composite / native {tc / tn:5.2f} "
          f"| kernel {tk:8.1f} us (spread {100 * sk:4.1f} %) {flops / tk / 1e6:6.0f} TOP/s | native faster by more than the composite's spread: "
          f"{'yes' if wins else 'no'} | rule -> {'native' if rule else 'composite'} | pool {pool} | max rel diff {err:.1e}", flush=True)
    return wins


def bench_linear(cfg, dname, M, N, K, iters, repeats):
    fmt, bs, sf = CONFIGS[cfg]
    dtype = DTYPES[dname]
    el = 2 if dtype == torch.bfloat16 else 4
    per_set = (M * K + N * K + M * N) * el + (M + N) * K
    pool = int(max(2, min(16, POOL_BYTES // per_set + 1)))
    g = torch.Generator(device=DEV).manual_seed(0)
    acts, weights, packed = [], [], []
    for _ in range(pool):
        x = (torch.randn((M, K), generator=g, device=DEV) * 2).to(dtype)
        w = (torch.randn((N, K), generator=g, device=DEV) * 0.05).to(dtype)
        acts.append(quantized(x, fmt, bs, -1, sf))
        weights.append(quantized(w, fmt, bs, -1, sf))
    del x, w

    def native(i):
        j = i % pool
        return torch.ops.quantized_ops.linear_mx(acts[j][0], weights[j][0], None, input_scale=acts[j][1], weight_scale=weights[j][1], block_size=bs)
    native(0)
    for j in range(pool):
        q, s = acts[j]
        packed.append((mx_gemm._int_pack(q, s, None, bs, 1, M, K, (0, K, 1), (0, K // bs, 1), False),
                       mx_gemm._int_weight_operand(weights[j][0], weights[j][1], None, bs)))
    out = torch.empty((M, N), dtype=dtype, device=DEV)

    def kernel(i):
        pa, pb = packed[i % pool]
        return mx_gemm._int_gemm(pa, pb, bs, out, None, 1, M, N, K, 0, 0, out)
    return report(f"linear_mx {dname} {cfg} {M}x{N}x{K}", 2.0 * M * N * K, native, composite_of(native), kernel, iters, repeats, pool,
                  mx_gemm._int_route_takes(M, N, K, 1, bs, dtype))


def bench_matmul(which, dname, iters, repeats):
    fmt, bs, sf = CONFIGS["int6,bs=64"]
    dtype = DTYPES[dname]
    B, H, S, D = 1, 32, 1024, 128
    g = torch.Generator(device=DEV).manual_seed(1)
    pool = 4
    sets = []
    for _ in range(pool):
        if which == "Q.K^T":
            a0 = torch.randn((B, H, S, D), generator=g, device=DEV).to(dtype)
            b0 = torch.randn((B, H, S, D), generator=g, device=DEV).to(dtype).transpose(-1, -2)
        else:
            a0 = torch.rand((B, H, S, S), generator=g, device=DEV).to(dtype)
            b0 = torch.randn((B, H, S, D), generator=g, device=DEV).to(dtype)
        sets.append(quantized(a0, fmt, bs, -1, sf) + quantized(b0, fmt, bs, -2, sf))
    M, K = sets[0][0].shape[-2:]
    N = sets[0][2].shape[-1]

    def native(i):
        a, sa, b, sb = sets[i % pool]
        return torch.ops.quantized_ops.matmul_mx(a, b, input_scale=sa, weight_scale=sb, block_size=bs)
    packed = []
    for a, sa, b, sb in sets:
        pa = mx_gemm._int_pack(a.contiguous(), sa.contiguous(), None, bs, B * H, M, K, (M * K, K, 1), (M * (K // bs), K // bs, 1), False)
        b3, xb = mx_gemm._rows_view(b, B * H, N, K)
        s3, xs = mx_gemm._rows_view(sb, B * H, N, K // bs)
        packed.append((pa, mx_gemm._int_pack(b3, s3, None, bs, B * H, N, K, xb, xs, False)))
    out = torch.empty((B, H, M, N), dtype=dtype, device=DEV)

    def kernel(i):
        pa, pb = packed[i % pool]
        return mx_gemm._int_gemm(pa, pb, bs, out, None, B * H, M, N, K, M, N, out)
    return report(f"matmul_mx {dname} int6,bs=64 {which} [{B},{H},{M},{K}] x [{B},{H},{K},{N}]", 2.0 * B * H * M * N * K, native, composite_of(native),
                  kernel, iters, repeats, pool, mx_gemm._int_route_takes(M, N, K, B * H, bs, dtype))


def kernel_by_block_size(iters, repeats):
    M, N, K = 1024, 4096, 4096
    g = torch.Generator(device=DEV).manual_seed(2)
    a = torch.randint(-31, 32, (1, M, K), generator=g, device=DEV, dtype=torch.int8)
    b = torch.randint(-31, 32, (1, N, K), generator=g, device=DEV, dtype=torch.int8)
    out = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    fns = {}
    for bs in (32, 64, 128):
        sa = torch.rand((1, M, K // bs), generator=g, device=DEV) + 0.5
        sb = torch.rand((1, N, K // bs), generator=g, device=DEV) + 0.5
        fns[bs] = (lambda i, sa=sa, sb=sb, bs=bs: mx_gemm._int_gemm((a, sa), (b, sb), bs, out, None, 1, M, N, K, 0, 0, out))
    t = rounds(fns, iters, repeats)
    for bs in (32, 64, 128):
        print(f"# kernel alone, bf16 out, {M}x{N}x{K}, bs = {bs:3d}: {t[bs][0]:8.1f} us (spread {100 * t[bs][1]:4.1f} %) {2.0 * M * N * K / t[bs][0] / 1e6:6.0f} TOP/s",
              flush=True)
    print(f"# time(bs = 64) / time(bs = 128) = {t[64][0] / t[128][0]:.2f}, time(bs = 32) / time(bs = 64) = {t[32][0] / t[64][0]:.2f}   (same matrix "
          f"instructions for 64 and 128, half the conversions / scale products / fmas: a ratio near 2 means the vector pipe bounds the kernel)", flush=True)


def main():
    mx_gemm._APPLY_INT_RULE = False                                 # time every row on every route, a declined class included
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; the operators linear_mx / matmul_mx on integer operands; median of {args.repeats} "
          f"rounds of {args.iters} calls per route, routes alternating (spread = (max - min) / median)", flush=True)
    classes = {}
    for cfg in ("int6,bs=64,scale=fp8_e5m3", "int8,bs=32"):
        for dname in DTYPES:
            for M, N, K in LINEARS:
                classes.setdefault(f"projections {dname}", []).append(bench_linear(cfg, dname, M, N, K, args.iters, args.repeats))
    for dname in DTYPES:
        for which in ("Q.K^T", "P.V"):
            classes.setdefault(f"attention matmuls {dname}", []).append(bench_matmul(which, dname, args.iters, args.repeats))
    for dname in DTYPES:
        for M, N, K in SMALL:
            classes.setdefault(f"small linears {dname}", []).append(bench_linear("int8,bs=32", dname, M, N, K, 20 * args.iters, args.repeats))
        for M, N, K in MID:
            classes.setdefault(f"in between {dname}", []).append(bench_linear("int8,bs=32", dname, M, N, K, 5 * args.iters, args.repeats))
    for name, wins in classes.items():
        print(f"# {name}: native faster than the composite by more than the composite's spread on {sum(wins)} of {len(wins)} rows", flush=True)
    kernel_by_block_size(args.iters, args.repeats)


if __name__ == "__main__":
    main()
