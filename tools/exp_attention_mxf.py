"""Route timings of the block-scaled float attention core: the span of nodes as a converted graph runs it today against the
attention_mx operator on the kernel route (any pack inside the timed call; quantize_mx's packed operands are read in place), in ONE
process, the two routes alternating, medians of 9 (min - max spread next to them) after warming every shape, eager and replayed from a
graph, with a causal mask and without a mask, and the peak temporaries of one call of each route.  Prints the rows of
profiles/attention_mxf.txt's timing section and, behind them, one verdict per class (B, H, Q, C, D): it clears the bar of
mx_attention._MXF_ATTENTION_TABLE when the kernel route's median beats the nodes' by more than the nodes' min - max spread eager AND
replayed, with AND without the mask, for fp8_e4m3 AND fp4_e2m1.

    python tools/exp_attention_mxf.py [--once]     (on an MI355X; fails without a GPU.  --once: one kernel-route call per shape and
                                                    format and nothing else, the run a kernel trace is taken of)
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "quantized-training_amd")]
from quantized_training.fake_quantize import get_quantization_map  # noqa: E402

OPS = torch.ops.quantized_ops
SHAPES = [(1, 32, 128, 512), (1, 32, 128, 1024), (1, 32, 128, 2048), (1, 32, 128, 4096), (4, 12, 64, 512), (4, 12, 64, 2048)]   # B, H, D, S
FORMATS = [("fp8_e4m3", 448.0), ("fp4_e2m1", 6.0)]
WINDOW_MS = 40.0                                                                                # a timed window is at least this long


def time_us(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / inner


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    once = "--once" in sys.argv
    verdict = {}                                                                                # (B, H, Q, C, D) -> every setting cleared
    for (B, H, D, S), (fmt, qmax) in ((s, f) for s in SHAPES for f in FORMATS):
        torch.manual_seed(0)
        qm = get_quantization_map(fmt, dev)
        x = [torch.randn(B, H, S, D, device=dev).bfloat16() for _ in range(3)]
        qs, qq = OPS.quantize_mx(x[0], qm, [-1], 32, qmax, True, None, None)
        ks, kq = OPS.quantize_mx(x[1].transpose(-1, -2), qm, [-2], 32, qmax, True, None, None)
        vs, vq = OPS.quantize_mx(x[2], qm, [-2], 32, qmax, True, None, None)
        causal = torch.full((S, S), float("-inf"), device=dev).triu(1).bfloat16()[None, None]
        c = D ** -0.5

        def nodes(mask):
            s = OPS.matmul_mx(qq, kq, input_scale=qs, weight_scale=ks, block_size=32) * c
            if mask is not None:
                s = s + mask
            ps, pq = OPS.quantize_mx(torch.softmax(s, -1), qm, [-1], 32, qmax, True, None, None)
            return OPS.matmul_mx(pq, vq, input_scale=ps, weight_scale=vs, block_size=32)

        def kernel(mask):
            os.environ["QT_FUSED_ATTENTION"] = "1"
            try:
                return OPS.attention_mx(qq, qs, kq, ks, vq, vs, mask, c, False, qm, qmax, True, None, False, 32)
            finally:
                del os.environ["QT_FUSED_ATTENTION"]

        if once:
            kernel(causal)
            torch.cuda.synchronize()
            continue
        for mask, mname in ((causal, "causal"), (None, "no mask")):
            routes = {"nodes": lambda: nodes(mask), "kernel": lambda: kernel(mask)}
            err = (routes["kernel"]().float() - routes["nodes"]().float()).abs().max().item()
            peaks = {}
            for name, fn in routes.items():
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fn()
                torch.cuda.synchronize()
                peaks[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            for mode in ("eager", "replayed"):
                calls = dict(routes)
                if mode == "replayed":
                    for name, fn in routes.items():
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            fn()
                        calls[name] = g.replay
                inner = {}
                for name, fn in calls.items():                                  # warm-up of both routes; the window's length from it
                    time_us(fn, 3)
                    inner[name] = max(5, int(WINDOW_MS * 1000.0 / time_us(fn, 5)) + 1)
                t = {name: [] for name in calls}
                for _ in range(9):                                              # alternating
                    for name, fn in calls.items():
                        t[name].append(time_us(fn, inner[name]))
                med = {n: statistics.median(v) for n, v in t.items()}
                spread = {n: max(v) - min(v) for n, v in t.items()}
                clears = med["nodes"] - med["kernel"] > spread["nodes"]
                verdict[(B, H, S, S, D)] = verdict.get((B, H, S, S, D), True) and clears
                print(f"{fmt} B {B} H {H} D {D} S {S} {mname:8s} {mode:8s} nodes {med['nodes']:9.1f} us (spread {spread['nodes']:.1f}) "
                      f"kernel {med['kernel']:9.1f} us (spread {spread['kernel']:.1f})  clears {clears}  peak MiB nodes {peaks['nodes']:.1f} kernel "
                      f"{peaks['kernel']:.1f}  max |kernel - nodes| {err:.4g}", flush=True)
    for shape, ok in verdict.items():
        print(f"class (B, H, Q, C, D) = {shape}: {'clears the bar in every setting' if ok else 'does not clear the bar'}", flush=True)


if __name__ == "__main__":
    main()
