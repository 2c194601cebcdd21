"""conv2d_q, both routes in one process on one box: the operator on the integer matrix instruction (qt_quantize_codes_nhwc_* +
qt_q8_conv2d, through quantized_training/pt2e_native.py) against the graph it replaces -- quantize to a value tensor, the library's
convolution on two value tensors, dequantize -- on ResNet-50's body layers at batch 32 in bf16 (the shapes of profiles/conv2d_mx.txt).

The baseline runs twice, with an NCHW-contiguous activation and with a channels_last one (what a layer behind a native convolution
receives); so does the candidate, whose codes pass is inside the timed call (a transposition for NCHW, a straight pass for
channels_last).  The weight is stored as the two graphs store it: bf16 values [Cout, Cin, kh, kw] for the baseline, int8 codes
[Cout, kh, kw, Cin] for the candidate.  Operands rotate over a pool larger than the Infinity Cache.  Timing: warm-up, then REPEATS
rounds; a round times ITERS calls of each route between two events, the routes alternating inside the round; per route the median of
the rounds with their min and max -- once with eager calls (the host's dispatch of three operators against one is part of the
time) and once with the ITERS calls of each route recorded into a hipGraph that a round replays (device time alone).  A row clears
the bar only when the native median beats the baseline median by more than the baseline's own min-max spread for both layouts in
both modes.  One more route is timed for what it costs, not for the bar: conv2d_q made to decline, i.e. the operator's predicate and
bookkeeping in front of the same three nodes on the stored parameter -- what a layer pays that the rule keeps with the graph.
The table this prints is committed as profiles/conv2d_q.txt and decides
pt2e_native._conv_q_route_takes (the tool switches the rule off so that every layer is timed on every route).

    timeout -k 10 900 python tools/exp_conv_q.py [--iters 100] [--repeats 7]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
from quantized_training import pt2e_native  # noqa: E402
from quantized_training.fake_quantize import get_quantization_map  # noqa: E402

DEV = "cuda:0"
POOL_BYTES = 320e6            # > the 256 MB Infinity Cache
BATCH = 32
# (H = W, Cin, Cout, k): ResNet-50 body layers, stride 1, padding k // 2
SHAPES = [(56, 64, 64, 3), (28, 128, 128, 3), (14, 256, 256, 3), (7, 512, 512, 3), (56, 64, 64, 1), (56, 64, 256, 1), (56, 256, 64, 1),
          (28, 128, 512, 1), (28, 512, 128, 1), (14, 256, 1024, 1), (14, 1024, 256, 1), (7, 512, 2048, 1), (7, 2048, 512, 1)]
# (batch, H = W, Cin, Cout, k): what the layers above do not cover -- the narrowest Cin the kernel takes, a few hundred output pixels
# (a grid of two to four tiles), a 7 x 7 filter
EXTRA = [(4, 14, 32, 64, 3), (4, 7, 64, 64, 3), (4, 7, 512, 512, 3), (4, 14, 256, 64, 1), (32, 28, 32, 64, 7)]


def rounds(fns, iters, repeats, captured):
    """{name: (median, min, max)} in us per call; the routes alternate inside every round.  captured: the ITERS calls of a route are
    recorded into one hipGraph and a round replays it, which takes the host's dispatch out of the time."""
    for fn in fns.values():
        for i in range(5):
            fn(i)
    torch.cuda.synchronize()
    graphs = {}
    if captured:
        for name, fn in fns.items():
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for i in range(iters):
                    fn(i)
            graphs[name].replay()
        torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for r in range(repeats):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            if captured:
                graphs[name].replay()
            else:
                for i in range(iters):
                    fn(r * iters + i)
            e.record()
            torch.cuda.synchronize()
            out[name].append(s.elapsed_time(e) * 1e3 / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def bench(batch, hw, cin, cout, k, iters, repeats):
    pad = k // 2
    qmap = get_quantization_map("int8", DEV)
    per_set = batch * hw * hw * (cin * 2 * 2 + cout * 2) + cout * k * k * cin * 3
    pool = int(max(2, min(48, POOL_BYTES // per_set + 1)))
    g = torch.Generator(device=DEV).manual_seed(0)
    s_x = torch.tensor(0.03, device=DEV).bfloat16()
    s_out = torch.tensor([2e-4], device=DEV).bfloat16()
    nchw, nhwc, values, codes, biases = [], [], [], [], []
    for _ in range(pool):
        x = (torch.randn((batch, cin, hw, hw), generator=g, device=DEV) * 1.2).bfloat16()
        wq = torch.randint(-127, 128, (cout, cin, k, k), generator=g, device=DEV)
        nchw.append(x); nhwc.append(x.contiguous(memory_format=torch.channels_last))
        values.append(wq.bfloat16()); codes.append(wq.permute(0, 2, 3, 1).contiguous().to(torch.int8))
        codes[-1]._qt_conv_values = values[-1]                        # as the pass leaves it: a declined call convolves the stored parameter
        biases.append(torch.randint(-2000, 2000, (cout,), generator=g, device=DEV).bfloat16())
    quantize, dequantize, conv_q = torch.ops.quantized_ops.quantize, torch.ops.quantized_ops.dequantize, torch.ops.quantized_ops.conv2d_q

    def baseline(src):
        def run(i):
            j = i % pool
            xq = quantize(src[j], s_x, None, None, None, qmap)
            return dequantize(F.conv2d(xq, values[j], biases[j], 1, pad), s_out, None, None, None, None)
        return run

    def native(src):
        def run(i):
            j = i % pool
            return conv_q(src[j], s_x, qmap, codes[j], biases[j], [1, 1], [pad, pad], [1, 1], 1, s_out, None, "int8")
        return run

    def declined(src):
        """conv2d_q as a layer the route rule keeps with the graph runs it: the predicate, the bookkeeping, then the three nodes."""
        def run(i):
            j = i % pool
            keep = pt2e_native._APPLY_CONV_Q_RULE, pt2e_native._conv_q_route_takes
            pt2e_native._APPLY_CONV_Q_RULE, pt2e_native._conv_q_route_takes = True, lambda *a: False
            try:
                return conv_q(src[j], s_x, qmap, codes[j], biases[j], [1, 1], [pad, pad], [1, 1], 1, s_out, None, "int8")
            finally:
                pt2e_native._APPLY_CONV_Q_RULE, pt2e_native._conv_q_route_takes = keep
        return run

    before = pt2e_native.STATS["conv2d_int8"]
    y, ref = native(nchw)(0), baseline(nchw)(0)
    y2 = native(nhwc)(0)
    assert pt2e_native.STATS["conv2d_int8"] - before == 2, f"the native route declined this shape: {pt2e_native.CONV_Q_REASONS}"
    assert torch.equal(y, y2)
    assert torch.equal(declined(nchw)(0), ref) and pt2e_native.STATS["conv2d_int8"] - before == 2
    err = (y.float() - ref.float()).abs().max().item() / ref.float().abs().max().item()
    fns = {"base nchw": baseline(nchw), "native nchw": native(nchw), "base nhwc": baseline(nhwc), "native nhwc": native(nhwc),
           "declined nchw": declined(nchw)}
    wins = []
    cells = []
    for mode, captured in (("eager", False), ("replay", True)):
        t = rounds(fns, iters, repeats, captured)
        for lay in ("nchw", "nhwc"):
            (bm, blo, bhi), (nm, nlo, nhi) = t[f"base {lay}"], t[f"native {lay}"]
            wins.append(bm - nm > bhi - blo)
            cells.append(f"{mode} {lay}: graph {bm:6.1f} us [{blo:6.1f}, {bhi:6.1f}] conv2d_q {nm:6.1f} us [{nlo:6.1f}, {nhi:6.1f}] ratio {bm / nm:4.2f}")
        dm, dlo, dhi = t["declined nchw"]
        cells.append(f"{mode} nchw conv2d_q declined (the three nodes inside the operator) {dm:6.1f} us [{dlo:6.1f}, {dhi:6.1f}]")
    flops = 2.0 * batch * hw * hw * cout * cin * k * k
    rule = pt2e_native._conv_q_route_takes(batch * hw * hw, cout, cin, k, k)
    print(f"{batch}x{cin}x{hw}x{hw} -> {cout} {k}x{k} | " + " | ".join(cells) + f" | {flops / t['native nhwc'][0] / 1e6:5.0f} TOP/s (replay nhwc, "
          f"codes pass included) | clears the bar: {'yes' if all(wins) else 'no'} | rule -> {'native' if rule else 'graph'} | pool {pool} "
          f"| max rel diff {err:.1e}", flush=True)
    return all(wins), rule


def main():
    pt2e_native._APPLY_CONV_Q_RULE = False                          # time every layer on both routes, declined classes included
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    assert args.repeats >= 5
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; int8 per-tensor, bf16 model; graph = quantize + aten.conv2d + dequantize, "
          f"conv2d_q = codes pass + qt_q8_conv2d; median [min, max] of {args.repeats} rounds of {args.iters} calls per route, routes alternating, "
          f"eager calls and hipGraph replays; bar: graph median - conv2d_q median > graph max - graph min, on both layouts in both modes",
          flush=True)
    odd = []
    for s in [(BATCH, *s) for s in SHAPES] + EXTRA:
        wins, rule = bench(*s, args.iters, args.repeats)
        if wins != bool(rule):
            odd.append(s)
    print(f"# rows where the committed rule and the bar disagree: {odd}", flush=True)


if __name__ == "__main__":
    main()
