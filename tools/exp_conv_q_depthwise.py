"""conv2d_q on its depthwise and narrow pointwise routes against the graph it replaces, both in one process on one box: the method of
tools/exp_conv_q.py on MobileNetV2's shapes at batch 32 in bf16.

Depthwise rows: the operator (qt_quantize_codes_nhwc_* + qt_q8_dwconv2d) against quantize to a value tensor, the library's grouped
convolution on two value tensors, dequantize.  Pointwise rows (1 x 1, stride 1, Cin = 16 mod 32): the operator (codes pass + qt_q8_gemm)
against the same three nodes.  Each route runs with an NCHW-contiguous activation and with a channels_last one; the codes pass is inside
the timed call.  The weight is stored as the two graphs store it: bf16 values for the baseline, int8 codes [Cout, kh, kw, Cin / groups] for
the candidate.  Operands rotate over a pool larger than the Infinity Cache.  Timing: warm-up, then REPEATS rounds; a round times ITERS
calls of each route between two events, the routes alternating inside the round; per route the median of the rounds with their min and
max -- once with eager calls and once with the ITERS calls of each route recorded into a hipGraph that a round replays.  A row clears
the bar only when the native median beats the baseline median by more than the baseline's own min-max spread for both layouts in both
modes.  Depthwise rows also time qt_q8_dwconv2d alone on codes made beforehand (replayed), for its bytes per second: codes read once plus
the bf16 result written once, next to the 6.29 TB/s of a float4 copy on this chip.
The table this prints is committed as profiles/conv2d_q_depthwise.txt and decides pt2e_native._conv_q_dw_route_takes and
_conv_q_pw16_route_takes (the tool switches the rules off so that every layer is timed on every route).

    timeout -k 10 900 python tools/exp_conv_q_depthwise.py [--iters 100] [--repeats 7]
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

# (batch, H = W, C, k, stride): MobileNetV2's depthwise layers at batch 32, one 5 x 5 layer, two batch-4 problems; padding k // 2
DEPTHWISE = [(32, 112, 32, 3, 1), (32, 112, 96, 3, 2), (32, 56, 144, 3, 1), (32, 56, 144, 3, 2), (32, 28, 192, 3, 1), (32, 28, 192, 3, 2),
             (32, 14, 384, 3, 1), (32, 14, 576, 3, 1), (32, 14, 576, 3, 2), (32, 7, 960, 3, 1), (32, 28, 240, 5, 1), (4, 56, 144, 3, 1),
             (4, 14, 576, 3, 1)]
# (batch, H = W, Cin, Cout): its pointwise layers over Cin = 16 mod 32
POINTWISE = [(32, 112, 16, 96), (32, 56, 144, 24), (32, 28, 144, 32)]


def bench(kind, batch, hw, cin, cout, k, stride, iters, repeats):
    depthwise = kind == "depthwise"
    pad, groups = k // 2, cin if depthwise else 1
    ho = (hw + 2 * pad - k) // stride + 1
    qmap = get_quantization_map("int8", DEV)
    per_set = batch * hw * hw * cin * 2 * 2 + batch * ho * ho * cout * 2 + cout * k * k * (cin // groups) * 3
    pool = int(max(2, min(48, POOL_BYTES // per_set + 1)))
    g = torch.Generator(device=DEV).manual_seed(0)
    s_x = torch.tensor(0.03, device=DEV).bfloat16()
    s_out = torch.tensor([2e-4], device=DEV).bfloat16()
    nchw, nhwc, values, codes, biases, made = [], [], [], [], [], []
    for _ in range(pool):
        x = (torch.randn((batch, cin, hw, hw), generator=g, device=DEV) * 1.2).bfloat16()
        wq = torch.randint(-127, 128, (cout, cin // groups, k, k), generator=g, device=DEV)
        nchw.append(x); nhwc.append(x.contiguous(memory_format=torch.channels_last))
        values.append(wq.bfloat16()); codes.append(wq.permute(0, 2, 3, 1).contiguous().to(torch.int8))
        codes[-1]._qt_conv_values = values[-1]                        # as the pass leaves it: a declined call convolves the stored parameter
        biases.append(torch.randint(-2000, 2000, (cout,), generator=g, device=DEV).bfloat16())
        if depthwise:
            made.append(pt2e_native.conv_codes_nhwc(nhwc[-1], s_x, qmap))
    quantize, dequantize, conv_q = torch.ops.quantized_ops.quantize, torch.ops.quantized_ops.dequantize, torch.ops.quantized_ops.conv2d_q
    geo = ([stride, stride], [pad, pad], [1, 1], groups)

    def baseline(src):
        def run(i):
            j = i % pool
            xq = quantize(src[j], s_x, None, None, None, qmap)
            return dequantize(F.conv2d(xq, values[j], biases[j], stride, pad, 1, groups), s_out, None, None, None, None)
        return run

    def native(src):
        def run(i):
            j = i % pool
            return conv_q(src[j], s_x, qmap, codes[j], biases[j], *geo, s_out, None, "int8")
        return run

    def declined(src):
        """conv2d_q as a layer the route rules keep with the graph runs it: the predicate, the bookkeeping, then the three nodes."""
        def run(i):
            j = i % pool
            keep = pt2e_native._APPLY_CONV_Q_RULE, pt2e_native._conv_q_dw_route_takes, pt2e_native._conv_q_pw16_route_takes
            pt2e_native._APPLY_CONV_Q_RULE = True
            pt2e_native._conv_q_dw_route_takes = pt2e_native._conv_q_pw16_route_takes = lambda *a: False
            try:
                return conv_q(src[j], s_x, qmap, codes[j], biases[j], *geo, s_out, None, "int8")
            finally:
                pt2e_native._APPLY_CONV_Q_RULE, pt2e_native._conv_q_dw_route_takes, pt2e_native._conv_q_pw16_route_takes = keep
        return run

    out = torch.empty((batch, cout, ho, ho), dtype=torch.bfloat16, device=DEV, memory_format=torch.channels_last)

    def kernel_alone(i):
        j = i % pool
        rc = _native.lib().qt_q8_dwconv2d(made[j].data_ptr(), codes[j].data_ptr(), out.data_ptr(), 0, biases[j].data_ptr(), s_out.data_ptr(), 0, 0,
                                          batch, hw, hw, cin, k, k, stride, stride, pad, pad, 1, 1, _stream_ptr(out))
        assert rc == 0, rc

    key = "conv2d_dw_int8" if depthwise else "conv2d_int8"
    before = pt2e_native.STATS[key]
    y, ref = native(nchw)(0), baseline(nchw)(0)
    y2 = native(nhwc)(0)
    assert pt2e_native.STATS[key] - before == 2, f"the native route declined this shape: {pt2e_native.CONV_Q_REASONS}"
    assert torch.equal(y, y2)
    assert torch.equal(declined(nchw)(0), ref) and pt2e_native.STATS[key] - before == 2
    err = (y.float() - ref.float()).abs().max().item() / ref.float().abs().max().item()
    fns = {"base nchw": baseline(nchw), "native nchw": native(nchw), "base nhwc": baseline(nhwc), "native nhwc": native(nhwc),
           "declined nchw": declined(nchw)}
    if depthwise:
        fns["kernel"] = kernel_alone
    wins, cells = [], []
    for mode, captured in (("eager", False), ("replay", True)):
        t = rounds(fns, iters, repeats, captured)
        for lay in ("nchw", "nhwc"):
            (bm, blo, bhi), (nm, nlo, nhi) = t[f"base {lay}"], t[f"native {lay}"]
            wins.append(bm - nm > bhi - blo)
            cells.append(f"{mode} {lay}: graph {bm:6.1f} us [{blo:6.1f}, {bhi:6.1f}] conv2d_q {nm:6.1f} us [{nlo:6.1f}, {nhi:6.1f}] ratio {bm / nm:4.2f}")
        dm, dlo, dhi = t["declined nchw"]
        cells.append(f"{mode} nchw conv2d_q declined (the three nodes inside the operator) {dm:6.1f} us [{dlo:6.1f}, {dhi:6.1f}]")
    m = batch * ho * ho
    if depthwise:
        km, klo, khi = t["kernel"]
        nbytes = batch * hw * hw * cin + m * cin * 2
        rule = pt2e_native._conv_q_dw_route_takes(m, cin, k, k, stride, stride)
        head = f"depthwise {batch}x{cin}x{hw}x{hw} {k}x{k} stride {stride}"
        tail = f"qt_q8_dwconv2d alone (replay) {km:6.1f} us [{klo:6.1f}, {khi:6.1f}] = {nbytes / km / 1e6:4.2f} TB/s of codes read + bf16 written (copy: 6.29)"
    else:
        rule = pt2e_native._conv_q_pw16_route_takes(m, cout, cin)
        head = f"pointwise {batch}x{cin}x{hw}x{hw} -> {cout}"
        tail = f"{2.0 * m * cout * cin / t['native nhwc'][0] / 1e6:5.1f} TOP/s (replay nhwc, codes pass included)"
    print(f"{head} | " + " | ".join(cells) + f" | {tail} | clears the bar: {'yes' if all(wins) else 'no'} | rule -> "
          f"{'native' if rule else 'graph'} | pool {pool} | max rel diff {err:.1e}", flush=True)
    return all(wins), rule


def main():
    pt2e_native._APPLY_CONV_Q_RULE = False                          # time every layer on both routes, declined classes included
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    assert args.repeats >= 5
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; int8 per-tensor, bf16 model; graph = quantize + aten.conv2d + dequantize, "
          f"conv2d_q = codes pass + qt_q8_dwconv2d (depthwise rows) or qt_q8_gemm (pointwise rows); median [min, max] of {args.repeats} rounds of "
          f"{args.iters} calls per route, routes alternating, eager calls and hipGraph replays; bar: graph median - conv2d_q median > graph max - "
          f"graph min, on both layouts in both modes", flush=True)
    odd = []
    for b, hw, c, k, s in DEPTHWISE:
        wins, rule = bench("depthwise", b, hw, c, c, k, s, args.iters, args.repeats)
        if rule and not wins:
            odd.append(("depthwise", b, hw, c, k, s))
    for b, hw, cin, cout in POINTWISE:
        wins, rule = bench("pointwise", b, hw, cin, cout, 1, 1, args.iters, args.repeats)
        if rule and not wins:
            odd.append(("pointwise", b, hw, cin, cout))
    print(f"# rows the committed rules send to the native route although they did not clear the bar: {odd}", flush=True)


if __name__ == "__main__":
    main()
