"""Chained converted int8 convolutions against the un-chained native graph, both in one process on one box: the method and the bar of
tools/exp_conv_q.py on MobileNetV2's expand -> ReLU6 -> depthwise -> ReLU6 -> project chains and one ResNet-50 bottleneck at batch 32 in
bf16.

Un-chained (the graph convert_pt2e returns today): conv2d_q -> aten.hardtanh / aten.relu -> conv2d_q -> ... : every layer rounds its sums
to bf16 and writes them, the activation reads and writes them, the next layer's codes pass reads them again.  Chained
(fuse_conv_q_chains): the same layers as conv2d_qc nodes -- the producer's epilogue applies the activation and the consumer's quantize
and writes 1 B codes (qt_q8_*_codes), the consumer gathers them.  The first layer takes a channels_last bf16 activation (the layout a
native layer in front of it leaves), the last one writes bf16 values; both routes must give the same bits.  Where a network's expand
layer is one no kernel takes (Cin = 24), the chain starts at the depthwise layer.  Operands rotate over a pool larger than the Infinity
Cache.  Timing: tools/exp_conv_q.rounds -- warm-up, then REPEATS rounds; a round times ITERS calls of each route between two events, the
routes alternating; medians with min and max, once with eager calls and once with the calls recorded into a hipGraph.  A chain clears the
bar when the chained median beats the un-chained median by more than the un-chained route's own min-max spread in both modes.
The table is printed and written to profiles/conv2d_q_chain.txt (the tool switches the route rules off so that every chain is timed;
the last column says whether the committed rules would let the pass chain it).

    timeout -k 10 900 python tools/exp_conv_q_chain.py [--iters 50] [--repeats 7]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from exp_conv_q import DEV, POOL_BYTES, rounds  # noqa: E402
from quantized_training import pt2e_native  # noqa: E402
from quantized_training.fake_quantize import get_quantization_map  # noqa: E402

RELU6, RELU = (0.0, 6.0), (0.0, None)
# (name, batch, H = W, Cin, [(Cout, k, stride, groups)], activation between the layers)
CHAINS = [
    ("mbv2 16-96-dw/2-24 @112", 32, 112, 16, [(96, 1, 1, 1), (96, 3, 2, 96), (24, 1, 1, 1)], RELU6),
    ("mbv2 dw144-24 @56", 32, 56, 144, [(144, 3, 1, 144), (24, 1, 1, 1)], RELU6),
    ("mbv2 dw144/2-32 @56", 32, 56, 144, [(144, 3, 2, 144), (32, 1, 1, 1)], RELU6),
    ("mbv2 32-192-dw-32 @28", 32, 28, 32, [(192, 1, 1, 1), (192, 3, 1, 192), (32, 1, 1, 1)], RELU6),
    ("mbv2 32-192-dw/2-64 @28", 32, 28, 32, [(192, 1, 1, 1), (192, 3, 2, 192), (64, 1, 1, 1)], RELU6),
    ("mbv2 64-384-dw-64 @14", 32, 14, 64, [(384, 1, 1, 1), (384, 3, 1, 384), (64, 1, 1, 1)], RELU6),
    ("mbv2 96-576-dw-96 @14", 32, 14, 96, [(576, 1, 1, 1), (576, 3, 1, 576), (96, 1, 1, 1)], RELU6),
    ("mbv2 96-576-dw/2-160 @14", 32, 14, 96, [(576, 1, 1, 1), (576, 3, 2, 576), (160, 1, 1, 1)], RELU6),
    ("mbv2 160-960-dw-160 @7", 32, 7, 160, [(960, 1, 1, 1), (960, 3, 1, 960), (160, 1, 1, 1)], RELU6),
    ("resnet50 256-64-3x3-256 @56", 32, 56, 256, [(64, 1, 1, 1), (64, 3, 1, 1), (256, 1, 1, 1)], RELU),
]


def bench(name, batch, hw, cin, layers, bounds, iters, repeats):
    qmap = get_quantization_map("int8", DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    sizes, h, c = [], hw, cin
    for cout, k, stride, groups in layers:
        h = (h + 2 * (k // 2) - k) // stride + 1
        sizes.append(batch * h * h * cout)
        c = cout
    per_set = batch * hw * hw * cin * 2 + sum(sizes) * 2
    pool = int(max(2, min(48, POOL_BYTES // per_set + 1)))
    s_x = [torch.tensor(0.03, device=DEV).bfloat16() for _ in layers]
    s_out = [torch.tensor([2e-4 * (9 if groups > 1 else 1)], device=DEV).bfloat16() for _, _, _, groups in layers]
    xs, weights = [], []
    for _ in range(pool):
        xs.append((torch.randn((batch, cin, hw, hw), generator=g, device=DEV) * 1.2).bfloat16().contiguous(memory_format=torch.channels_last))
        ws, c = [], cin
        for cout, k, stride, groups in layers:
            wq = torch.randint(-127, 128, (cout, c // groups, k, k), generator=g, device=DEV)
            codes = wq.permute(0, 2, 3, 1).contiguous().to(torch.int8)
            codes._qt_conv_values = wq.bfloat16()
            ws.append((codes, torch.randint(-2000, 2000, (cout,), generator=g, device=DEV).bfloat16()))
            c = cout
        weights.append(ws)
    conv_q, conv_qc = torch.ops.quantized_ops.conv2d_q, torch.ops.quantized_ops.conv2d_qc
    geo = [([s, s], [k // 2, k // 2], [1, 1], groups) for _, k, s, groups in layers]
    last = len(layers) - 1

    def plain(i):
        j = i % pool
        y = xs[j]
        for n, (codes, bias) in enumerate(weights[j]):
            y = conv_q(y, s_x[n], qmap, codes, bias, *geo[n], s_out[n], None, "int8")
            if n < last:
                y = torch.relu(y) if bounds == RELU else F.hardtanh(y, *bounds)
        return y

    def chained(i):
        j = i % pool
        y = xs[j]
        for n, (codes, bias) in enumerate(weights[j]):
            head = (y, s_x[n], qmap) if n == 0 else (y, None, None)
            tail = (*bounds, s_x[n + 1], qmap) if n < last else (None, None, None, None)
            y = conv_qc(*head, codes, bias, *geo[n], s_out[n], None, "int8", *tail)
        return y

    before, reasons = dict(pt2e_native.STATS), sum(pt2e_native.CONV_Q_REASONS.values())
    want, got = plain(0), chained(0)
    assert torch.equal(want, got), "the chained route and the un-chained route disagree"
    assert pt2e_native.STATS["conv2d_codes_out"] - before["conv2d_codes_out"] == last and sum(pt2e_native.CONV_Q_REASONS.values()) == reasons, \
        f"a layer of the chain fell back: {pt2e_native.CONV_Q_REASONS}"
    fns = {"plain": plain, "chained": chained}
    wins, cells = [], []
    for mode, captured in (("eager", False), ("replay", True)):
        t = rounds(fns, iters, repeats, captured)
        (pm, plo, phi), (cm, clo, chi) = t["plain"], t["chained"]
        wins.append(pm - cm > phi - plo)
        cells.append(f"{mode}: un-chained {pm:6.1f} us [{plo:6.1f}, {phi:6.1f}] chained {cm:6.1f} us [{clo:6.1f}, {chi:6.1f}] ratio {pm / cm:4.2f}")
    # what the committed rules say about every layer of the chain as a device call
    pt2e_native._APPLY_CONV_Q_RULE = True
    try:
        ruled, shape, c = True, (batch, cin, hw, hw), cin
        for n, (cout, k, stride, groups) in enumerate(layers):
            x = pt2e_native._Operand(shape, torch.bfloat16, DEV)
            why = pt2e_native._conv_q_decline(x, s_x[n], qmap, weights[0][n][0], weights[0][n][1], *geo[n], s_out[n], "int8", on_device=True)
            ruled = ruled and why is None
            ho = (shape[2] + 2 * (k // 2) - k) // stride + 1
            shape = (batch, cout, ho, ho)
    finally:
        pt2e_native._APPLY_CONV_Q_RULE = False
    saved = sum(sizes[:-1]) * 8                                      # per handed-over element: 2 + 2 + 2 + 2 + 1 B become 1 B
    line = (f"{name} x{batch} | " + " | ".join(cells) + f" | {saved / 1e6:6.1f} MB of traffic and {2 * last} launches fewer per call | clears the "
            f"bar: {'yes' if all(wins) else 'no'} | the committed route rules take every layer: {'yes' if ruled else 'no'} | pool {pool}")
    print(line, flush=True)
    return line, all(wins)


def main():
    pt2e_native._APPLY_CONV_Q_RULE = False                          # time every chain, whatever the route rules say about its layers
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv2d_q_chain.txt"))
    args = ap.parse_args()
    assert args.repeats >= 5
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; int8 per-tensor, bf16 model, channels_last input; un-chained = conv2d_q -> "
             f"aten.hardtanh(0, 6) / aten.relu -> conv2d_q ..., chained = the same layers as conv2d_qc nodes handing over int8 codes; median [min, max] "
             f"of {args.repeats} rounds of {args.iters} calls per route, routes alternating, eager calls and hipGraph replays; bar: un-chained median - "
             f"chained median > un-chained max - un-chained min, in both modes"]
    print(lines[0], flush=True)
    lost = []
    for chain in CHAINS:
        line, wins = bench(*chain, args.iters, args.repeats)
        lines.append(line)
        if not wins:
            lost.append(chain[0])
    lines.append(f"# chains that did not clear the bar: {lost}")
    print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
