"""The split of K of the native int8 convolution (qt_q8_conv2d_ws, csrc/qt_mx_conv.hip), all routes in one process on one box:
reducing 1 x 1 and few-tile layers, the shapes on which profiles/conv2d_q.txt shows the unsplit kernel losing to the graph.

Per row, in bf16: the three nodes of the converted graph (quantize + aten.conv2d + dequantize) on an NCHW-contiguous and on a
channels_last activation; conv2d_q on an UNMARKED codes buffer (the unsplit kernel, exactly the parent commit's route); conv2d_q on a
marked buffer with the split forced to every S of the candidate set that the shape admits (S <= nk), and with the plan's S
(qt_q8_conv2d_plan).  Each from both layouts, the codes pass inside the timed call, and once from codes arriving from a producer
(conv2d_qc with a code array as input: the launch alone, what a chained layer costs).  The method is tools/exp_conv_q.py's: operands
rotate over a pool larger than the Infinity Cache; warm-up, then REPEATS rounds in which the routes alternate, a round timing ITERS
calls of each route between two events; median [min, max] per route, for eager calls and for hipGraph replays.

The bar is the one of profiles/conv2d_q.txt: the native median must beat the three nodes' median by more than the three nodes' own
min - max spread, in both layouts and both modes.  It is evaluated for the plan's S (the route a marked layer takes) and printed for
the unsplit kernel and every forced S as well.  The table this prints is committed as profiles/conv2d_q_splitk.txt; it decides
pt2e_native._conv_q_split_route_takes and the plan's constants (kConvSplitSet, kConvSplitMinKTiles in csrc/qt_mx_conv.hip).

    timeout -k 10 900 python tools/exp_conv_q_splitk.py [--iters 50] [--repeats 7] [--rows resnet,batch4,mobilenet]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
from quantized_training import _native, pt2e_native  # noqa: E402
from quantized_training.fake_quantize import get_quantization_map  # noqa: E402

DEV = "cuda:0"
POOL_BYTES = 320e6            # > the 256 MB Infinity Cache
CANDIDATES = (2, 4, 8, 16)
SLAB = 65536
# (batch, H = W, Cin, Cout, k), stride 1, padding k // 2
ROWS = {
    "resnet": [(32, 56, 256, 64, 1), (32, 28, 512, 128, 1), (32, 14, 1024, 256, 1), (32, 7, 2048, 512, 1), (32, 7, 512, 512, 3)],
    "batch4": [(4, 14, 32, 64, 3), (4, 7, 64, 64, 3), (4, 7, 512, 512, 3), (4, 14, 256, 64, 1)],
    "mobilenet": [(32, 28, 192, 32, 1), (32, 14, 192, 64, 1), (32, 14, 384, 64, 1), (32, 14, 384, 96, 1), (32, 14, 576, 96, 1),
                  (32, 7, 576, 160, 1), (32, 7, 960, 160, 1), (32, 7, 960, 320, 1)],
}

_PLAN = _native.q8_conv_plan
_forced = [0]                 # 0: the plan's split


def _plan(m, cout, k):
    """What _conv_q_launch asks for a marked layer: the committed plan, or the forced split with the workspace it needs."""
    if _forced[0] == 0:
        return _PLAN(m, cout, k)
    tiles = -(-m // 128) * -(-cout // 128)
    s = _forced[0]
    return (s, tiles * s * SLAB, tiles) if s > 1 else (1, 0, 0)


def rounds(fns, iters, repeats, captured):
    """{name: (median, min, max)} in us per call; the routes alternate inside every round (tools/exp_conv_q.py)."""
    for fn in fns.values():
        for i in range(3):
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
    m, kk = batch * hw * hw, k * k * cin
    tiles, nk = -(-m // 128) * -(-cout // 128), -(-kk // 128)
    qmap = get_quantization_map("int8", DEV)
    per_set = batch * hw * hw * (cin * 2 * 2 + cin + cout * 2) + cout * kk * 4
    pool = int(max(2, min(48, POOL_BYTES // per_set + 1)))
    g = torch.Generator(device=DEV).manual_seed(0)
    s_x = torch.tensor(0.03, device=DEV).bfloat16()
    s_out = torch.tensor([2e-4], device=DEV).bfloat16()
    nchw, nhwc, xcodes, values, plain, marked, biases = [], [], [], [], [], [], []
    for _ in range(pool):
        x = (torch.randn((batch, cin, hw, hw), generator=g, device=DEV) * 1.2).bfloat16()
        wq = torch.randint(-127, 128, (cout, cin, k, k), generator=g, device=DEV)
        nchw.append(x); nhwc.append(x.contiguous(memory_format=torch.channels_last))
        xcodes.append(pt2e_native.conv_codes_nhwc(x, s_x, qmap).view(batch, hw, hw, cin).permute(0, 3, 1, 2))
        values.append(wq.bfloat16())
        plain.append(wq.permute(0, 2, 3, 1).contiguous().to(torch.int8))
        marked.append(pt2e_native.mark_split_k(plain[-1].clone()))
        biases.append(torch.randint(-2000, 2000, (cout,), generator=g, device=DEV).bfloat16())
    quantize, dequantize = torch.ops.quantized_ops.quantize, torch.ops.quantized_ops.dequantize
    conv_q, conv_qc = torch.ops.quantized_ops.conv2d_q, torch.ops.quantized_ops.conv2d_qc
    geo = ([1, 1], [pad, pad], [1, 1], 1)

    def baseline(src):
        def run(i):
            j = i % pool
            xq = quantize(src[j], s_x, None, None, None, qmap)
            return dequantize(F.conv2d(xq, values[j], biases[j], 1, pad), s_out, None, None, None, None)
        return run

    def native(src, weights, split):
        def run(i):
            j = i % pool
            _forced[0] = split
            if src is xcodes:
                return conv_qc(src[j], None, None, weights[j], biases[j], *geo, s_out, None, "int8", None, None, None, None)
            return conv_q(src[j], s_x, qmap, weights[j], biases[j], *geo, s_out, None, "int8")
        return run

    plan_s = _PLAN(m, cout, kk)[0]
    splits = [s for s in CANDIDATES if s <= nk]
    ref = native(nchw, plain, 0)(0)
    before = pt2e_native.STATS["conv2d_split_k"]
    for s in splits:                                           # every forced split computes what the unsplit kernel computes
        for src in (nchw, nhwc, xcodes):
            assert torch.equal(native(src, marked, s)(0), ref), (s, pt2e_native.CONV_Q_REASONS)
    assert pt2e_native.STATS["conv2d_split_k"] - before == 3 * len(splits), pt2e_native.CONV_Q_REASONS
    fns = {"base nchw": baseline(nchw), "base nhwc": baseline(nhwc)}
    for lay, src in (("nchw", nchw), ("nhwc", nhwc), ("codes", xcodes)):
        fns[f"S=1 {lay}"] = native(src, plain, 0)
        for s in splits:
            fns[f"S={s} {lay}"] = native(src, marked, s)
    head = f"{batch}x{cin}x{hw}x{hw} -> {cout} {k}x{k} | tiles {tiles} nk {nk} plan S={plan_s}"
    clears = {s: [] for s in [1] + splits}
    lines = []
    for mode, captured in (("eager", False), ("replay", True)):
        t = rounds(fns, iters, repeats, captured)
        for lay in ("nchw", "nhwc", "codes"):
            bm, blo, bhi = t[f"base {'nhwc' if lay == 'codes' else lay}"]
            cells = [f"graph {bm:6.1f} [{blo:6.1f}, {bhi:6.1f}]" if lay != "codes" else "(launch alone)             "]
            for s in [1] + splits:
                nm, nlo, nhi = t[f"S={s} {lay}"]
                cells.append(f"S={s} {nm:6.1f} [{nlo:6.1f}, {nhi:6.1f}]" + (f" {bm / nm:4.2f}x" if lay != "codes" else ""))
                if lay != "codes":
                    clears[s].append(bm - nm > bhi - blo)
            lines.append(f"    {mode:6s} {lay:5s} us: " + " | ".join(cells))
    verdict = " ".join(f"S={s}:{'yes' if all(v) else 'no'}" for s, v in clears.items())
    plan_clears = all(clears[plan_s])
    rule = pt2e_native._conv_q_split_route_takes(m, cout, cin, k, k) or pt2e_native._conv_q_route_takes(m, cout, cin, k, k)
    print(f"{head} | clears the bar: {verdict} | plan clears the bar: {'yes' if plan_clears else 'no'} | marked layer -> "
          f"{'native' if rule else 'graph'} | pool {pool}", flush=True)
    for line in lines:
        print(line, flush=True)
    return plan_clears, rule


def chains_under_the_rules():
    """The ten chains of tools/exp_conv_q_chain.py under the committed rules, every gather layer marked (convert_pt2e(split_k=True)):
    which layers the rules take, the split the plan gives each, whether fuse_conv_q_chains would chain it end to end.  A predicate
    on shapes (the one the pass evaluates); nothing is timed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from exp_conv_q_chain import CHAINS
    s1, qmap = pt2e_native._Operand((1,), torch.bfloat16, DEV), pt2e_native._Operand((65536,), torch.bfloat16, DEV)
    s_out = torch.ones(1, dtype=torch.bfloat16)
    whole = {False: 0, True: 0}
    for name, batch, hw, cin, layers, _ in CHAINS:
        cells = {False: [], True: []}
        for marked in (False, True):
            shape, c = (batch, cin, hw, hw), cin
            for cout, k, stride, groups in layers:
                w = torch.zeros((cout, k, k, c // groups), dtype=torch.int8)
                if marked and groups == 1 and c % 32 == 0:
                    pt2e_native.mark_split_k(w)
                why = pt2e_native._conv_q_decline(pt2e_native._Operand(shape, torch.bfloat16, DEV), s1, qmap, w, None, [stride, stride],
                                                  [k // 2, k // 2], [1, 1], groups, s_out, "int8", on_device=True)
                ho = (shape[2] + 2 * (k // 2) - k) // stride + 1
                split = _PLAN(batch * ho * ho, cout, k * k * c)[0] if pt2e_native._split_k_marked(w) else 1
                cells[marked].append(f"{c}->{cout} {k}x{k}{'/dw' if groups > 1 else ''}: {'native' if why is None else 'graph'}" + (f" S={split}" if split > 1 else ""))
                shape, c = (batch, cout, ho, ho), cout
            whole[marked] += all("native" in cell for cell in cells[marked])
        print(f"chain {name} x{batch} | rules on, unmarked: {'; '.join(cells[False])} | rules on, split_k=True: {'; '.join(cells[True])} | chains end to "
              f"end: {'yes' if all('native' in c for c in cells[True]) else 'no'}", flush=True)
    print(f"# chains the committed rules let fuse_conv_q_chains chain end to end: {whole[False]} of {len(CHAINS)} unmarked, {whole[True]} of "
          f"{len(CHAINS)} with split_k=True; a chain whose layers keep their routes and splits keeps the times of profiles/conv2d_q_chain.txt",
          flush=True)


def main():
    pt2e_native._APPLY_CONV_Q_RULE = False                          # time every layer on every route
    _native.q8_conv_plan = _plan
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", default="resnet,batch4,mobilenet")
    args = ap.parse_args()
    assert args.repeats >= 5
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# {torch.cuda.get_device_name(0)}, {cus} CUs; torch {torch.__version__}; int8 per-tensor, bf16 model; graph = quantize + aten.conv2d + "
          f"dequantize; S=1 = conv2d_q on an unmarked layer (codes pass + qt_q8_conv2d, the unsplit kernel); S>1 = a marked layer with the split "
          f"forced (codes pass + qt_q8_conv2d_ws); codes = conv2d_qc on a producer's code array (the launch alone); median [min, max] us of "
          f"{args.repeats} rounds of {args.iters} calls per route, routes alternating, eager calls and hipGraph replays; bar: graph median - "
          f"native median > graph max - graph min, on both layouts in both modes", flush=True)
    odd = []
    for group in args.rows.split(","):
        for s in ROWS[group]:
            clears, rule = bench(*s, args.iters, args.repeats)
            if rule and not clears:
                odd.append(s)
    print(f"# rows a marked layer takes natively although the plan's split did not clear the bar: {odd}", flush=True)
    pt2e_native._APPLY_CONV_Q_RULE = True
    _forced[0] = 0
    chains_under_the_rules()


if __name__ == "__main__":
    main()
