"""A packed group-wise affine Linear at M > 32, the routes of linear_gwa in one process on one box:

    (b) gwa_dequantize    qt_gwa_dequantize_bf16 (writes a bf16 copy of the weight on every call) + aten.linear
    (t) tall              qt_linear_gwa_tall_bf16 at its plan's row tile and split (csrc/qt_gwa_tall.hip): no copy of the weight
    (c) fused             qt_linear_gwa_bf16, forced, for M <= 128 (csrc/qt_gwa_gemm.hip: every 64 rows convert the weight again)

Rows: uint4 and uint8, bs = 128, on LLaMA-2-7B's projections (N x K = 4096 x 4096, 11008 x 4096, 4096 x 11008) at M = 64 .. 2048.  The packed weights, scales and zero points rotate over a pool larger than the Infinity Cache, so every call reads its
weight from memory, as a layer of a model does.  Timing as in tools/exp_gwa_linear.py: warm-up, then REPEATS rounds; a round times
ITERS calls of each route between two events, the routes alternating inside the round; min / median / max of the rounds.  The bar is
that file's: (t)'s SLOWEST round must beat the FASTEST round of (b).  A class -- the rows of one M and one code width -- enters
pt2e_native._gwa_tall_route_takes only where every weight of the class clears it.  The table this prints is committed as
profiles/gwa_tall.txt.

    timeout -k 10 900 python tools/exp_gwa_tall.py [--iters 20] [--repeats 7]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_gwa_linear import DEV, POOL_BYTES, rounds  # noqa: E402
from quantized_training import _native, pt2e_native as pn  # noqa: E402

BS, QMIN = 128, 0
WEIGHTS = [(b, n, k) for b in (4, 8) for n, k in ((4096, 4096), (11008, 4096), (4096, 11008))]      # bits, N, K
TOKENS = [64, 96, 128, 192, 256, 384, 512, 1024, 2048]


def pool_of(bits, N, K):
    """Packed weights (any byte string is a valid operand), scales and zero points, more of them than the Infinity Cache holds."""
    g = torch.Generator(device=DEV).manual_seed(N + K + bits)
    span = 16 if bits == 4 else 256
    first = pn.gwa_pack(torch.randint(0, span, (N, K), device=DEV, generator=g).to(torch.bfloat16), 0, span - 1, bits)
    n = max(2, int(POOL_BYTES // first.numel()) + 1)
    packed = [first] + [torch.randint(0, 256, first.shape, device=DEV, generator=g, dtype=torch.uint8) for _ in range(n - 1)]
    scale = [(torch.rand(N, K // BS, device=DEV, generator=g) * 0.02 + 0.001).to(torch.bfloat16) for _ in range(n)]
    zero = [(torch.rand(N, K // BS, device=DEV, generator=g) * (span - 1)).to(torch.bfloat16) for _ in range(n)]
    return packed, scale, zero


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    print("# output of tools/exp_gwa_tall.py on one MI355X (python tools/exp_gwa_tall.py); pt2e_native._gwa_tall_route_takes rests on the column '(t) max < (b) min'")
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; bs=128 weights, bf16 activations; min / median / max of {args.repeats} rounds of "
          f"{args.iters} calls per route, routes alternating; weights rotate over > {POOL_BYTES / 1e6:.0f} MB")
    verdicts = {}
    for bits, N, K in WEIGHTS:
        packed, scale, zero = pool_of(bits, N, K)
        bias = torch.randn(N, device=DEV).to(torch.bfloat16)
        for M in TOKENS:
            x = torch.randn(M, K, device=DEV).to(torch.bfloat16)

            def route(name):
                def call(i):
                    j = i % len(packed)
                    return pn.linear_gwa_route(x, packed[j], scale[j], zero[j], bias, BS, QMIN, bits, K, route=name)
                return call
            fns = {"b": route("dequant"), "t": route("tall")}
            if M <= 128:
                fns["c"] = route("fused")
            yb, yt = fns["b"](0).float(), fns["t"](0).float()
            rel = float((yt - yb).abs().max() / yb.abs().max())
            r = rounds(fns, args.iters, args.repeats)
            fmt = lambda v: f"{v[0]:8.1f} /{v[1]:8.1f} /{v[2]:8.1f} us"      # noqa: E731
            wins = r["t"][2] < r["b"][0]
            verdicts.setdefault((bits, M), []).append(wins)
            bm, ks, wbytes, _ = _native.gwa_tall_plan(M, N, K, bits)
            line = (f"uint{bits} | {M:5d} x {N:5d} x {K:5d} | (b) gwa_dequantize + linear {fmt(r['b'])} | (t) tall, tile {bm:3d} split {ks} {fmt(r['t'])} | "
                    f"(b) / (t) {r['b'][1] / r['t'][1]:5.2f} | (t) max < (b) min: {'yes' if wins else 'no':3s} | "
                    f"rule -> {'tall' if pn._gwa_tall_route_takes(M, N, K, bits) else 'gwa_dequantize'} | workspace {wbytes / 1e6:5.1f} MB | (t) max rel diff {rel:.1e}")
            if "c" in r:
                line += f" | (c) fused, forced {fmt(r['c'])}"
            print(line, flush=True)
        del packed, scale, zero
        torch.cuda.empty_cache()
    for (bits, M), got in verdicts.items():
        print(f"# class uint{bits}, M = {M}: tall slowest round beats (b)'s fastest on {sum(got)} of {len(got)} weights -> {'clears the bar' if all(got) else 'loses'}")


if __name__ == "__main__":
    main()
