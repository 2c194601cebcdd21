"""Route timings of the block-scaled integer attention core: the span of nodes as a converted graph runs it today against the
attention_mx operator on the kernel route (its three qt_mxi_pack launches inside the timed call), in ONE process, the two routes
alternating, medians of 9 (min - max spread next to them), eager and replayed from a graph, with a causal mask and without a mask, and
the peak temporaries of one call of each route.  Prints the rows of profiles/attention_mxi.txt's timing section and, behind them, one
verdict per class (B, H, Q, C, D): it clears the bar of mx_attention._MXI_ATTENTION_TABLE when the kernel route's median beats the nodes'
by more than the nodes' min - max spread eager AND replayed, with AND without the mask, in every row measured at that shape.

    python tools/exp_attention_mxi.py          (on an MI355X; fails without a GPU)
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "quantized-training_amd")]
from quantized_training.fake_quantize import get_quantization_map  # noqa: E402

OPS = torch.ops.quantized_ops
SHAPES = [(1, 32, 128, 512, False), (1, 32, 128, 1024, False), (1, 32, 128, 2048, False), (1, 32, 128, 4096, False),
          (4, 12, 64, 512, False), (4, 12, 64, 2048, False), (1, 32, 128, 2048, True)]          # B, H, D, S, power-of-two scales
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
    qm, sm = get_quantization_map("int6", dev), get_quantization_map("fp8_e5m3", dev)
    verdict = {}                                                                                # (B, H, Q, C, D) -> every setting cleared
    for B, H, D, S, pow2 in SHAPES:
        torch.manual_seed(0)
        smap = None if pow2 else sm
        x = [torch.randn(B, H, S, D, device=dev).bfloat16() for _ in range(3)]
        qs, qq = OPS.quantize_mx(x[0], qm, [-1], 64, 31.0, pow2, smap, None)
        ks, kq = OPS.quantize_mx(x[1].transpose(-1, -2), qm, [-2], 64, 31.0, pow2, smap, None)
        vs, vq = OPS.quantize_mx(x[2], qm, [-2], 64, 31.0, pow2, smap, None)
        causal = torch.full((S, S), float("-inf"), device=dev).triu(1).bfloat16()[None, None]
        c = D ** -0.5

        def nodes(mask):
            s = OPS.matmul_mx(qq, kq, input_scale=qs, weight_scale=ks, block_size=64) * c
            if mask is not None:
                s = s + mask
            ps, pq = OPS.quantize_mx(torch.softmax(s, -1), qm, [-1], 64, 31.0, pow2, smap, None)
            return OPS.matmul_mx(pq, vq, input_scale=ps, weight_scale=vs, block_size=64)

        def kernel(mask):
            os.environ["QT_FUSED_ATTENTION"] = "1"
            try:
                return OPS.attention_mx(qq, qs, kq, ks, vq, vs, mask, c, False, qm, 31.0, pow2, smap, False, 64)
            finally:
                del os.environ["QT_FUSED_ATTENTION"]

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
                print(f"B {B} H {H} D {D} S {S} {'2^e' if pow2 else 'e5m3'} {mname:8s} {mode:8s} nodes {med['nodes']:9.1f} us (spread {spread['nodes']:.1f}) "
                      f"kernel {med['kernel']:9.1f} us (spread {spread['kernel']:.1f})  clears {clears}  peak MiB nodes {peaks['nodes']:.1f} kernel "
                      f"{peaks['kernel']:.1f}  max |kernel - nodes| {err:.4g}", flush=True)
    for shape, ok in verdict.items():
        print(f"class (B, H, Q, C, D) = {shape}: {'clears the bar in every setting' if ok else 'does not clear the bar'}", flush=True)


if __name__ == "__main__":
    main()
