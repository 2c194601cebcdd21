"""Group-wise affine kernels (csrc/qt_groupwise.hip) against the routes they replace, in one process.

Per shape, up to three routes take turns (warm-up first, then REPEATS rounds; in every round each route is timed once, over enough
calls to fill WINDOW_MS, between two device events):

  kernel     the fused HIP pass, through the module / the quantized_ops operator, exactly as a model calls it
  composite  the parent route: the torch-op composite (fake_quantize.group_wise_affine_composite; for dequantize the expand +
             subtract + multiply of decomposed._dequantize_impl)
  mx         last-axis fake-quant only: the microscaling module (qt_fake_quant_mx_bf16) on the same tensor and block size --
             the in-tree kernel with the same traffic

TB/s is algorithmic bytes (one read and one write of the tensor plus the block parameters) over the median time.  A route
"clears the bar" when its slowest repeat is faster than the composite's fastest.  Needs a GPU; writes the table to --out.

    python tools/exp_groupwise.py --out profiles/groupwise_fq.txt
"""
import argparse
import os
import statistics
import sys
from dataclasses import asdict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))

REPEATS = 5
WINDOW_MS = 60.0
POOL_BYTES = 512 << 20              # inputs rotate through a pool larger than the 256 MiB Infinity Cache


def module(spec):
    import quantized_training as qt
    return qt.FusedAmaxObsFakeQuantize(**asdict(qt.QuantizationSpec.from_str(spec)), device="cuda")


def timed(fn, pool, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(pool[i % len(pool)])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls              # ms per call


def measure(routes, pool):
    """routes: name -> callable(x).  Returns name -> sorted list of REPEATS per-call times in ms."""
    calls = {}
    for name, fn in routes.items():
        for x in pool:                               # warm-up on every input of the timed window
            fn(x)
        torch.cuda.synchronize()
        calls[name] = max(3, int(WINDOW_MS / max(timed(fn, pool, 3), 1e-3)))
    out = {name: [] for name in routes}
    for _ in range(REPEATS):
        for name, fn in routes.items():              # alternate the routes inside every round
            out[name].append(timed(fn, pool, calls[name]))
    return {k: sorted(v) for k, v in out.items()}


def fake_quant_row(label, shape, spec, mx_spec):
    from quantized_training.fake_quantize import group_wise_affine_composite
    numel = 1
    for d in shape:
        numel *= d
    pool = [torch.randn(shape, device="cuda").bfloat16() for _ in range(max(2, min(8, POOL_BYTES // (numel * 2))))]
    m = module(spec)
    ref = module(spec)
    routes = {"kernel": lambda x: m(x),
              "composite": lambda x: group_wise_affine_composite(x, ref.scale, ref.zero_point, ref.ch_axis, ref.block_size,
                                                                 ref.quant_min, ref.quant_max, ref.scale_qmap)}
    if mx_spec is not None:
        mx = module(mx_spec)
        routes["mx"] = lambda x: mx(x)
    y, yc = m(pool[0]), routes["composite"](pool[0])
    assert torch.equal(y.view(torch.int16), yc.view(torch.int16)) and torch.equal(m.scale, ref.scale) and \
        torch.equal(m.zero_point, ref.zero_point), f"{label}: the kernel and the composite disagree"
    nbytes = 2 * numel * 2 + 2 * (numel // m.block_size) * 2
    return label, nbytes, measure(routes, pool)


def dequantize_row(label, shape, spec):
    from quantized_training.decomposed import expand
    numel = shape[0] * shape[1]
    m = module(spec)
    pool, params = [], []
    for _ in range(max(2, min(8, POOL_BYTES // (numel * 2)))):
        w = torch.randn(shape, device="cuda").bfloat16()
        m(w)
        s, z = (t.to(w.dtype) for t in m.calculate_qparams())
        pool.append(torch.ops.quantized_ops.quantize(w, s, z, [-1], m.block_size, m.qmap))
        params.append((s, z))
    index = {id(x): p for x, p in zip(pool, params)}
    bs = m.block_size

    def kernel(x):
        s, z = index[id(x)]
        return torch.ops.quantized_ops.dequantize(x, s, z, [-1], bs)

    def composite(x):
        s, z = index[id(x)]
        return (x - expand(z, x.shape, bs)) * expand(s, x.shape, bs)

    assert torch.equal(kernel(pool[0]).view(torch.int16), composite(pool[0]).view(torch.int16)), f"{label}: routes disagree"
    nbytes = 2 * numel * 2 + 2 * (numel // bs) * 2
    return label, nbytes, measure({"kernel": kernel, "composite": composite}, pool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupwise_fq.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_groupwise.py measures on the GPU and there is none: nothing measured")
    torch.manual_seed(0)
    rows = []
    with torch.no_grad():
        rows.append(fake_quant_row("weight [11008,4096] bf16 uint4 bs=128 ax=-1", (11008, 4096), "uint4,qs=group_wise_affine,bs=128,ax=-1",
                                   "int4,qs=microscaling,bs=128,ax=-1"))
        rows.append(fake_quant_row("key [1,32,1024,128] bf16 uint2 bs=64 ax=-2 scale=fp8_e5m3", (1, 32, 1024, 128),
                                   "uint2,bs=64,qs=group_wise_affine,ax=-2,scale=fp8_e5m3", None))
        rows.append(fake_quant_row("value [1,32,1024,128] bf16 uint2 bs=64 ax=-1 scale=fp8_e5m3", (1, 32, 1024, 128),
                                   "uint2,bs=64,qs=group_wise_affine,ax=-1,scale=fp8_e5m3", "int4,qs=microscaling,bs=64,ax=-1"))
        rows.append(dequantize_row("dequantize weight [11008,4096] bf16 uint4 bs=128 ax=-1", (11008, 4096),
                                   "uint4,qs=group_wise_affine,bs=128,ax=-1"))
    lines = [f"# tools/exp_groupwise.py on {torch.cuda.get_device_name(0)}; {REPEATS} repeats per route, routes alternating, "
             f"{WINDOW_MS:.0f} ms windows between device events",
             "# time per call in microseconds: min / median / max; TB/s = algorithmic bytes / median",
             f"{'shape':<64} {'route':<10} {'min':>9} {'median':>9} {'max':>9} {'TB/s':>6}  verdict"]
    for label, nbytes, res in rows:
        parent_min = res["composite"][0]
        for name, t in res.items():
            med = statistics.median(t)
            verdict = ""
            if name == "kernel":
                verdict = "clears the bar" if t[-1] < parent_min else "DOES NOT clear the bar"
                verdict += f" ({statistics.median(res['composite']) / med:.1f}x the composite"
                verdict += f", {statistics.median(res['mx']) / med:.2f}x the mx kernel's bandwidth)" if "mx" in res else ")"
            lines.append(f"{label:<64} {name:<10} {t[0] * 1e3:9.1f} {med * 1e3:9.1f} {t[-1] * 1e3:9.1f} {nbytes / (med * 1e-3) / 1e12:6.2f}  {verdict}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
