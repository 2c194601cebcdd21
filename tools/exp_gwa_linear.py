"""A `uint4,qs=group_wise_affine,bs=128,ax=-1` Linear of a converted graph, three routes in one process on one box:

    (a) dequantize        today's graph: quantized_ops.dequantize on the bf16 codes (qt_dequantize_blocks_bf16: reads 2 B, writes 2 B per
                          weight) + aten.linear
    (b) gwa_dequantize    qt_gwa_dequantize_bf16 on the packed codes (reads 0.5 B, writes 2 B per weight) + aten.linear
    (c) fused             qt_linear_gwa_bf16: the dequantized weight is formed in registers and never written (csrc/qt_gwa_gemm.hip)

Rows: LLaMA-2-7B's projections (N x K = 4096 x 4096, 11008 x 4096, 4096 x 11008) at M = 1, 16, 128, 1024 tokens (and 32, 64, where the fused
kernel's tile changes), plus another of its tile heights at M = 16 and 64.  The weights (codes or packed codes, scales, zero points) rotate over a pool
larger than the Infinity Cache, so every call reads its weight from memory, as a layer of a model does.  Timing: warm-up, then
REPEATS rounds; a round times ITERS calls of each route between two events, the routes alternating inside the round; min / median /
max of the rounds.  The bar for the fused route is the project's usual one: its SLOWEST round must beat the FASTEST round of (b).
The table this prints is committed as profiles/gwa_linear.txt and decides pt2e_native._gwa_route_takes.

    timeout -k 10 900 python tools/exp_gwa_linear.py [--iters 20] [--repeats 7]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
from quantized_training import pt2e_native as pn  # noqa: E402

DEV = "cuda:0"
POOL_BYTES = 320e6            # > the 256 MB Infinity Cache
BS, QMIN, BITS = 128, 0, 4
WEIGHTS = [(4096, 4096), (11008, 4096), (4096, 11008)]      # N, K
TOKENS = [1, 16, 32, 64, 128, 1024]
EXTRA_TILES = {16: (64,), 64: (16,)}                         # forced tile heights timed beside the kernel's own choice


def rounds(fns, iters, repeats):
    """{name: (min, median, max)} in us per call; the routes alternate inside every round."""
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
    return {k: (min(v), statistics.median(v), max(v)) for k, v in out.items()}


def pool_of(N, K):
    g = torch.Generator(device=DEV).manual_seed(N + K)
    n_codes = max(2, int(POOL_BYTES // (N * K * 2)) + 1)
    n_packed = max(2, int(POOL_BYTES // (N * K // 2)) + 1)
    codes = [torch.randint(0, 16, (N, K), device=DEV, generator=g).to(torch.bfloat16) for _ in range(n_codes)]
    packed = [pn.gwa_pack(codes[i % n_codes], 0, 15, BITS) for i in range(min(n_packed, 2 * n_codes))]
    while len(packed) < n_packed:                             # any byte string is a valid operand: 16 codes in 4 bits
        packed.append(torch.randint(0, 256, packed[0].shape, device=DEV, generator=g, dtype=torch.uint8))
    n_par = max(n_codes, n_packed)
    scale = [(torch.rand(N, K // BS, device=DEV, generator=g) * 0.02 + 0.001).to(torch.bfloat16) for _ in range(n_par)]
    zero = [(torch.rand(N, K // BS, device=DEV, generator=g) * 15).to(torch.bfloat16) for _ in range(n_par)]
    return codes, packed, scale, zero


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    print(f"# output of tools/exp_gwa_linear.py on one MI355X (python tools/exp_gwa_linear.py); pt2e_native._gwa_route_takes rests on the last two columns")
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; uint4 bs=128 weights, bf16 activations; min / median / max of {args.repeats} rounds of "
          f"{args.iters} calls per route, routes alternating; weights rotate over > {POOL_BYTES / 1e6:.0f} MB per route")
    verdicts = {}
    for N, K in WEIGHTS:
        codes, packed, scale, zero = pool_of(N, K)
        bias = torch.randn(N, device=DEV).to(torch.bfloat16)
        for M in TOKENS:
            x = torch.randn(M, K, device=DEV).to(torch.bfloat16)

            def route_a(i):
                j = i % len(codes)
                return F.linear(x, torch.ops.quantized_ops.dequantize(codes[j], scale[j], zero[j], (-1,), BS), bias)

            def route_b(i):
                j = i % len(packed)
                return pn.linear_gwa_route(x, packed[j], scale[j], zero[j], bias, BS, QMIN, BITS, K, route="dequant")

            def fused(tile):
                def call(i):
                    j = i % len(packed)
                    return pn.linear_gwa_route(x, packed[j], scale[j], zero[j], bias, BS, QMIN, BITS, K, route="fused", tile_m=tile)
                return call
            fns = {"a": route_a, "b": route_b, "c": fused(0)}
            for t in EXTRA_TILES[M] if M in EXTRA_TILES else ():
                fns[f"c{t}"] = fused(t)
            # the three routes compute the same thing (packed[0] is the pack of codes[0])
            ya, yb, yc = route_a(0).float(), route_b(0).float(), fused(0)(0).float()
            rel = float((yc - ya).abs().max() / ya.abs().max())
            same_b = bool(torch.equal(ya, yb))
            r = rounds(fns, args.iters, args.repeats)
            fmt = lambda v: f"{v[0]:8.1f} /{v[1]:8.1f} /{v[2]:8.1f} us"      # noqa: E731
            wins = r["c"][2] < r["b"][0]
            verdicts[(M, N, K)] = wins
            tile = pn._native.lib().qt_linear_gwa_tile(M)
            line = (f"{M:5d} x {N:5d} x {K:5d} | (a) dequantize + linear {fmt(r['a'])} | (b) gwa_dequantize + linear {fmt(r['b'])} | "
                    f"(c) fused, tile {tile:3d} {fmt(r['c'])} | (a) / (b) {r['a'][1] / r['b'][1]:5.2f} | (b) / (c) {r['b'][1] / r['c'][1]:5.2f} | "
                    f"(b) max < (a) min: {'yes' if r['b'][2] < r['a'][0] else 'no':3s} | (c) max < (b) min: {'yes' if wins else 'no':3s} | "
                    f"rule -> {'fused' if pn._gwa_route_takes(M, N, K) else 'gwa_dequantize'} | (b) == (a) bit for bit: {same_b} | (c) max rel diff {rel:.1e}")
            for k in fns:
                if k.startswith("c") and k != "c":
                    line += f" | tile {k[1:]:>3s} {fmt(r[k])}"
            print(line, flush=True)
        del codes, packed, scale, zero
        torch.cuda.empty_cache()
    for M in TOKENS:
        got = [verdicts[(M, n, k)] for n, k in WEIGHTS]
        print(f"# M = {M}: fused slowest round beats (b)'s fastest on {sum(got)} of {len(got)} weights")


if __name__ == "__main__":
    main()
