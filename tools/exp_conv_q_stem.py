"""conv2d_q on its stem route (Cin <= 4) against the graph it replaces, both in one process on one box: the method of tools/exp_conv_q.py
on the first layers of ResNet-50, MobileNetV2 and an 11 x 11 / 4 stem, in bf16.

Layer rows: the operator on a marked codes buffer (qt_quantize_codes_nhwc4_* + qt_q8_stem_conv2d) against quantize to a value tensor,
the library's convolution on two value tensors, dequantize.  Each route runs with an NCHW-contiguous activation and with a
channels_last one; the codes pass is inside the timed call.  The weight is stored as the two graphs store it: bf16 values for the
baseline, int8 codes [Cout, kh, kw, Cin] for the candidate.  Operands rotate over a pool larger than the Infinity Cache.  Timing:
tools/exp_conv_q.rounds -- warm-up, then REPEATS rounds; a round times ITERS calls of each route between two events, the routes
alternating inside the round; per route the median of the rounds with their min and max -- once with eager calls and once with the
ITERS calls of each route recorded into a hipGraph that a round replays.  A row clears the bar only when the native median beats the
baseline median by more than the baseline's own min-max spread for both layouts in both modes.  Each row also times qt_q8_stem_conv2d
alone on pixel dwords made beforehand (replayed), for its bytes per second: dwords read once plus the bf16 result written once.
Chain rows: MobileNetV2's stem -> ReLU6 -> depthwise 3 x 3, un-chained (conv2d_q, aten.hardtanh, conv2d_q) against chained (two
conv2d_qc nodes, the stem writing the depthwise layer's codes); the same bar in both modes, from both layouts.
The table is printed and written to profiles/conv2d_q_stem.txt and decides pt2e_native._conv_q_stem_route_takes (the tool switches the
rules off so that every row is timed on every route; the last column says what the committed rule does with the row).

    timeout -k 10 900 python tools/exp_conv_q_stem.py [--iters 50] [--repeats 7]
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
from quantized_training import _native, pt2e_native  # noqa: E402
from quantized_training.fake_quantize import _stream_ptr, get_quantization_map  # noqa: E402

# (name, batch, H = W, Cout, k, stride, padding) over 3 input channels
STEMS = [("resnet50 7x7/2 -> 64", 32, 224, 64, 7, 2, 3), ("resnet50 7x7/2 -> 64", 4, 224, 64, 7, 2, 3),
         ("mobilenetv2 3x3/2 -> 32", 32, 224, 32, 3, 2, 1), ("mobilenetv2 3x3/2 -> 32", 4, 224, 32, 3, 2, 1),
         ("11x11/4 -> 64", 32, 224, 64, 11, 4, 2)]
CHAINS = [("mobilenetv2 stem -> relu6 -> dw3x3", 32, 224, 32, 3, 2, 1), ("mobilenetv2 stem -> relu6 -> dw3x3", 4, 224, 32, 3, 2, 1)]
CIN = 3


def operands(batch, hw, cout, k, ho, with_dw):
    per_set = batch * hw * hw * CIN * 2 * 2 + batch * ho * ho * cout * (6 if with_dw else 2)
    pool = int(max(2, min(48, POOL_BYTES // per_set + 1)))
    g = torch.Generator(device=DEV).manual_seed(0)
    sets = []
    for _ in range(pool):
        x = (torch.randn((batch, CIN, hw, hw), generator=g, device=DEV) * 1.2).bfloat16()
        wq = torch.randint(-127, 128, (cout, CIN, k, k), generator=g, device=DEV)
        codes = pt2e_native.mark_stem(wq.permute(0, 2, 3, 1).contiguous().to(torch.int8))
        codes._qt_conv_values = wq.bfloat16()                          # as the pass leaves it: a declined call convolves the stored parameter
        dq = torch.randint(-127, 128, (cout, 1, 3, 3), generator=g, device=DEV)
        dw = dq.permute(0, 2, 3, 1).contiguous().to(torch.int8)
        dw._qt_conv_values = dq.bfloat16()
        sets.append(dict(nchw=x, nhwc=x.contiguous(memory_format=torch.channels_last), values=codes._qt_conv_values, codes=codes, dw=dw,
                         bias=torch.randint(-2000, 2000, (cout,), generator=g, device=DEV).bfloat16()))
    return sets


def bench_stem(name, batch, hw, cout, k, stride, pad, iters, repeats):
    ho = (hw + 2 * pad - k) // stride + 1
    qmap = get_quantization_map("int8", DEV)
    sets = operands(batch, hw, cout, k, ho, False)
    pool = len(sets)
    s_x, s_out = torch.tensor(0.03, device=DEV).bfloat16(), torch.tensor([2e-4], device=DEV).bfloat16()
    quantize, dequantize, conv_q = torch.ops.quantized_ops.quantize, torch.ops.quantized_ops.dequantize, torch.ops.quantized_ops.conv2d_q
    geo = ([stride, stride], [pad, pad], [1, 1], 1)
    made = [pt2e_native.conv_codes_nhwc(s["nhwc"], s_x, qmap, stem=True) for s in sets]
    out = torch.empty((batch, cout, ho, ho), dtype=torch.bfloat16, device=DEV, memory_format=torch.channels_last)

    def baseline(lay):
        def run(i):
            s = sets[i % pool]
            xq = quantize(s[lay], s_x, None, None, None, qmap)
            return dequantize(F.conv2d(xq, s["values"], s["bias"], stride, pad), s_out, None, None, None, None)
        return run

    def native(lay):
        def run(i):
            s = sets[i % pool]
            return conv_q(s[lay], s_x, qmap, s["codes"], s["bias"], *geo, s_out, None, "int8")
        return run

    def kernel_alone(i):
        j = i % pool
        rc = _native.lib().qt_q8_stem_conv2d(made[j].data_ptr(), sets[j]["codes"].data_ptr(), out.data_ptr(), 0, sets[j]["bias"].data_ptr(),
                                             s_out.data_ptr(), 0, 0, batch, hw, hw, CIN, cout, k, k, stride, stride, pad, pad, 1, 1, _stream_ptr(out))
        assert rc == 0, rc

    before = pt2e_native.STATS["conv2d_stem_int8"]
    y, y2, ref = native("nchw")(0), native("nhwc")(0), baseline("nchw")(0)
    assert pt2e_native.STATS["conv2d_stem_int8"] - before == 2, f"the native route declined this shape: {pt2e_native.CONV_Q_REASONS}"
    assert torch.equal(y, y2)
    err = (y.float() - ref.float()).abs().max().item() / ref.float().abs().max().item()
    fns = {"base nchw": baseline("nchw"), "native nchw": native("nchw"), "base nhwc": baseline("nhwc"), "native nhwc": native("nhwc"),
           "kernel": kernel_alone}
    wins, cells = [], []
    for mode, captured in (("eager", False), ("replay", True)):
        t = rounds(fns, iters, repeats, captured)
        for lay in ("nchw", "nhwc"):
            (bm, blo, bhi), (nm, nlo, nhi) = t[f"base {lay}"], t[f"native {lay}"]
            wins.append(bm - nm > bhi - blo)
            cells.append(f"{mode} {lay}: graph {bm:6.1f} us [{blo:6.1f}, {bhi:6.1f}] conv2d_q {nm:6.1f} us [{nlo:6.1f}, {nhi:6.1f}] ratio {bm / nm:4.2f}")
    km, klo, khi = t["kernel"]
    m = batch * ho * ho
    nbytes = batch * hw * hw * 4 + m * cout * 2
    rule = pt2e_native._conv_q_stem_route_takes(m, cout, CIN, k, k, stride, stride)
    line = (f"{name} {batch}x{CIN}x{hw}x{hw} | " + " | ".join(cells) + f" | qt_q8_stem_conv2d alone (replay) {km:6.1f} us [{klo:6.1f}, {khi:6.1f}] = "
            f"{nbytes / km / 1e6:4.2f} TB/s of dwords read + bf16 written | clears the bar: {'yes' if all(wins) else 'no'} | rule -> "
            f"{'native' if rule else 'graph'} | pool {pool} | max rel diff {err:.1e}")
    print(line, flush=True)
    return line, all(wins), rule


def bench_chain(name, batch, hw, cout, k, stride, pad, iters, repeats):
    ho = (hw + 2 * pad - k) // stride + 1
    qmap = get_quantization_map("int8", DEV)
    sets = operands(batch, hw, cout, k, ho, True)
    pool = len(sets)
    s_x, s_mid = torch.tensor(0.03, device=DEV).bfloat16(), torch.tensor(0.03, device=DEV).bfloat16()
    s_out, s_dw = torch.tensor([2e-4], device=DEV).bfloat16(), torch.tensor([2e-3], device=DEV).bfloat16()
    conv_q, conv_qc = torch.ops.quantized_ops.conv2d_q, torch.ops.quantized_ops.conv2d_qc
    geo, geo_dw = ([stride, stride], [pad, pad], [1, 1], 1), ([1, 1], [1, 1], [1, 1], cout)

    def plain(lay):
        def run(i):
            s = sets[i % pool]
            y = F.hardtanh(conv_q(s[lay], s_x, qmap, s["codes"], s["bias"], *geo, s_out, None, "int8"), 0.0, 6.0)
            return conv_q(y, s_mid, qmap, s["dw"], s["bias"], *geo_dw, s_dw, None, "int8")
        return run

    def chained(lay):
        def run(i):
            s = sets[i % pool]
            y = conv_qc(s[lay], s_x, qmap, s["codes"], s["bias"], *geo, s_out, None, "int8", 0.0, 6.0, s_mid, qmap)
            return conv_qc(y, None, None, s["dw"], s["bias"], *geo_dw, s_dw, None, "int8", None, None, None, None)
        return run

    before, reasons = dict(pt2e_native.STATS), sum(pt2e_native.CONV_Q_REASONS.values())
    assert torch.equal(plain("nchw")(0), chained("nchw")(0)), "the chained route and the un-chained route disagree"
    assert pt2e_native.STATS["conv2d_stem_int8"] - before["conv2d_stem_int8"] == 2 and pt2e_native.STATS["conv2d_codes_out"] - before["conv2d_codes_out"] == 1 \
        and sum(pt2e_native.CONV_Q_REASONS.values()) == reasons, f"a layer fell back: {pt2e_native.CONV_Q_REASONS}"
    fns = {f"{r} {lay}": f(lay) for lay in ("nchw", "nhwc") for r, f in (("plain", plain), ("chained", chained))}
    wins, cells = [], []
    for mode, captured in (("eager", False), ("replay", True)):
        t = rounds(fns, iters, repeats, captured)
        for lay in ("nchw", "nhwc"):
            (pm, plo, phi), (cm, clo, chi) = t[f"plain {lay}"], t[f"chained {lay}"]
            wins.append(pm - cm > phi - plo)
            cells.append(f"{mode} {lay}: un-chained {pm:6.1f} us [{plo:6.1f}, {phi:6.1f}] chained {cm:6.1f} us [{clo:6.1f}, {chi:6.1f}] ratio {pm / cm:4.2f}")
    line = f"{name} {batch}x{CIN}x{hw}x{hw} | " + " | ".join(cells) + f" | clears the bar: {'yes' if all(wins) else 'no'} | pool {pool}"
    print(line, flush=True)
    return line


def main():
    pt2e_native._APPLY_CONV_Q_RULE = False                          # time every row on both routes, whatever the rules say
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv2d_q_stem.txt"))
    args = ap.parse_args()
    assert args.repeats >= 5
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; int8 per-tensor, bf16 model; graph = quantize + aten.conv2d + dequantize, "
             f"conv2d_q = qt_quantize_codes_nhwc4_* + qt_q8_stem_conv2d on a marked codes buffer; chain rows: conv2d_q -> aten.hardtanh(0, 6) -> "
             f"depthwise conv2d_q against two conv2d_qc nodes; median [min, max] of {args.repeats} rounds of {args.iters} calls per route, routes "
             f"alternating, eager calls and hipGraph replays; bar: baseline median - candidate median > baseline max - baseline min, on both "
             f"layouts in both modes"]
    print(lines[0], flush=True)
    odd = []
    for row in STEMS:
        line, wins, rule = bench_stem(*row, args.iters, args.repeats)
        lines.append(line)
        if rule != wins:
            odd.append(row[:2])
    for row in CHAINS:
        lines.append(bench_chain(*row, args.iters, args.repeats))
    lines.append(f"# rows on which the committed rule and the bar disagree: {odd}")
    print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
