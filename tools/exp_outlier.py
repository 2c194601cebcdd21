"""The outlier side path, both routes in one process on one box: filter_outlier / spmm_csr on the kernels of csrc/qt_outlier.hip (through
quantized_training/outlier.py) against the torch composites they replace (QT_MX_GEMM=0: decomposed._filter_outlier_impl /
_spmm_csr_impl), on LLaMA-2-7B's projection shapes at 1024 tokens: activation [1024, 4096] into 4096 x 4096 and 11008 x 4096, activation
[1024, 11008] into 4096 x 11008.

The weight is what the converted graph passes: [N, K] values in the tensor's dtype with power-of-two block scales [N, K / 32].  Outliers
either sit in a few channels (the LLM case: whole columns scaled up) or are scattered uniformly (a threshold at the matching quantile of
|N(0, 1)|); their share is about 0.1 %, 1 % and just under the operator's 5 % cap (a truncated CSR makes the eager spmm_csr raise, as
upstream's loop does).  Both operators are called eagerly through torch.ops.quantized_ops, so the native route pays its 4-byte read of
indptr[-1] per call and the composite its own host reads.  Operands rotate over a pool larger than the Infinity Cache.  Timing:
warm-up, then REPEATS rounds; a round times ITERS calls of each of the four (operator, route) pairs between two events, the pairs
alternating inside the round; the median of the rounds with the spread (max - min) / median beside it.  The table this prints is
committed as profiles/outlier_path.txt.

    timeout -k 10 900 python tools/exp_outlier.py [--iters 4] [--repeats 5] [--dtypes bf16,f32]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
from quantized_training import outlier  # noqa: E402

DEV = "cuda:0"
POOL_BYTES = 320e6            # > the 256 MB Infinity Cache
TOKENS = 1024
SHAPES = [(4096, 4096), (4096, 11008), (11008, 4096)]          # (K of the activation, N of the weight)
SHARES = [0.001, 0.01, 0.048]
QUANTILE = {0.001: 3.296875, 0.01: 2.578125, 0.048: 1.9765625}       # |N(0, 1)| exceeds it with about that probability; bf16 numbers, so that
                                                                     # both routes compare with the same threshold in either dtype
ops = torch.ops.quantized_ops


def rounds(fns, iters, repeats):
    """{name: (median, spread)} in us per call; the routes alternate inside every round."""
    for fn in fns.values():
        for i in range(2):
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


def composite(fn):
    def call(i):
        os.environ["QT_MX_GEMM"] = "0"
        try:
            return fn(i)
        finally:
            os.environ["QT_MX_GEMM"] = "1"
    return call


def bench(dtype, K, N, share, pattern, iters, repeats):
    es = 2 if dtype == torch.bfloat16 else 4
    per_set = (TOKENS * K * 2 + N * K + TOKENS * N) * es
    pool = int(max(2, min(16, POOL_BYTES // per_set + 1)))
    g = torch.Generator(device=DEV).manual_seed(0)
    xs, ws, csrs = [], [], []
    for _ in range(pool):
        x = torch.randn((TOKENS, K), generator=g, device=DEV)
        if pattern == "channels":
            cols = torch.randperm(K, generator=g, device=DEV)[:max(1, round(share * K))]
            x[:, cols] *= 100.0
            threshold = 6.0
        else:
            threshold = QUANTILE[share]
        x = x.to(dtype)
        w = torch.randint(-127, 128, (N, K), generator=g, device=DEV).to(dtype)
        s = (2.0 ** torch.randint(-8, -3, (N, K // 32), generator=g, device=DEV).float()).to(dtype)
        xs.append(x); ws.append((w, s))
        csrs.append(ops.filter_outlier(x, threshold, 0.05)[1:])
        assert int(csrs[-1][2][-1]) <= csrs[-1][0].numel(), "the CSR is truncated: lower the share"
    nnz = int(csrs[0][2][-1])

    def flt(i):
        return ops.filter_outlier(xs[i % pool], threshold, 0.05)

    def spmm(i):
        j = i % pool
        return ops.spmm_csr(*csrs[j], ws[j][0], ws[j][1], None, 32)

    outlier.STATS.reset()
    y, ref = spmm(0), composite(spmm)(0)
    a, b = flt(0), composite(flt)(0)
    assert (outlier.STATS.native, outlier.STATS.fallback) == (2, 2), "a native route declined this shape"
    assert all(torch.equal(p, q) for p, q in zip(a, b)), "filter_outlier: the routes differ"
    err = (y.float() - ref.float()).abs().max().item() / ref.float().abs().max().item()
    t = rounds({"filter": flt, "filter composite": composite(flt), "spmm": spmm, "spmm composite": composite(spmm)}, iters, repeats)
    (tf, sf), (tfc, sfc), (ts, ss), (tsc, ssc) = t["filter"], t["filter composite"], t["spmm"], t["spmm composite"]
    name = "bf16" if dtype == torch.bfloat16 else "f32"
    print(f"{name} [{TOKENS}, {K}] x [{N}, {K}] {pattern:9s} nnz {nnz:6d} ({100 * nnz / (TOKENS * K):5.2f} %) "
          f"| filter: native {tf:8.1f} us (spread {100 * sf:4.1f} %), composite {tfc:8.1f} us (spread {100 * sfc:4.1f} %), composite / native {tfc / tf:6.2f} "
          f"| spmm: native {ts:8.1f} us (spread {100 * ss:4.1f} %), composite {tsc:9.1f} us (spread {100 * ssc:4.1f} %), composite / native {tsc / ts:7.2f} "
          f"| pair: composite / native {(tfc + tsc) / (tf + ts):7.2f} | pool {pool} | spmm max rel diff {err:.1e}", flush=True)
    return [op for op, native, comp, spread in (("filter", tf, tfc, sfc), ("spmm", ts, tsc, ssc)) if native > comp * (1.0 + spread)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,f32")
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; the operators filter_outlier (max_pct 0.05) and spmm_csr (block size 32), "
          f"eager; median of {args.repeats} rounds of {args.iters} calls per route, routes alternating (spread = (max - min) / median)", flush=True)
    slower = []
    for name in args.dtypes.split(","):
        dtype = {"bf16": torch.bfloat16, "f32": torch.float32}[name]
        for K, N in SHAPES:
            for pattern in ("channels", "scattered"):
                for share in SHARES:
                    for op in bench(dtype, K, N, share, pattern, args.iters, args.repeats):
                        slower.append((name, K, N, pattern, share, op))
    print(f"# native slower than the composite by more than the composite's spread on {len(slower)} rows: {slower}", flush=True)


if __name__ == "__main__":
    main()
