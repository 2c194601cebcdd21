"""Microscaling along an axis that is not the last (csrc/qt_mx_quant.hip, quantize_mx_strided_kernel) against the routes it
replaces, in one process.

Per row, the routes take turns (warm-up first, then REPEATS rounds; in every round each route is timed once, over enough calls to
fill WINDOW_MS, between two device events):

  kernel     through the quantized_ops operator or the fake-quant module, exactly as a model calls it; for the matmul rows the
             operand that matmul_mx reads (codes + E8M0 bytes) is part of the call
  parent     what ran before the kernel existed: the torch-op composite (calculate_mx_qparam + quantize, then q * expand(s) for the
             module), and for the matmul rows qt_mx_pack through strides on its result; for the transposed view also the
             .contiguous() copy the composite starts with.  The routes are switched off by name for the duration of a call.
  last-axis  the in-tree last-axis kernel (qt_quantize_mx_*) on the same tensor, blocks along axis -1: same traffic, for comparison

TB/s is algorithmic bytes (one read of the tensor, one write of the values, the block scales, and the packed operand where the row
has one) over the median time.  A route "clears the bar" when its slowest repeat is faster than the parent's fastest.
Needs a GPU; writes the table to --out.

    python tools/exp_mx_strided.py --out profiles/mx_strided.txt
"""
import argparse
import contextlib
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


@contextlib.contextmanager
def parent_routes():
    """The package as it ran before the strided kernel: every new route declines."""
    from quantized_training import decomposed, fake_quantize
    saved = (decomposed._quantize_mx_strided_hip_or_none, fake_quantize._hip_mx_strided_or_none, fake_quantize.transposed_storage)
    decomposed._quantize_mx_strided_hip_or_none = lambda *a, **k: None
    fake_quantize._hip_mx_strided_or_none = lambda *a, **k: None
    fake_quantize.transposed_storage = lambda t: None
    try:
        yield
    finally:
        decomposed._quantize_mx_strided_hip_or_none, fake_quantize._hip_mx_strided_or_none, fake_quantize.transposed_storage = saved


def as_parent(fn):
    def run(x):
        with parent_routes():
            return fn(x)
    return run


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


def make_pool(shape, dtype, view=None):
    numel = 1
    for d in shape:
        numel *= d
    n = max(2, min(8, POOL_BYTES // (numel * (2 if dtype == torch.bfloat16 else 4))))
    pool = [torch.randn(shape, device="cuda").to(dtype) for _ in range(n)]
    return [view(t) for t in pool] if view else pool, numel


def matmul_operand(q, s, bs):
    """The second operand of matmul_mx for q [..., K, N] with scales [..., K / bs, N], the way mx_gemm.mx_matmul_or_none gets it."""
    from quantized_training import mx_gemm, mx_operand
    fid = mx_gemm.FMT_ID[mx_operand.format_of(q)]
    K, N = q.shape[-2:]
    batch = q.numel() // (K * N)
    pre = mx_operand.operand(q, mx_operand.SECOND, fid, bs, batch * N, K)
    if pre is not None:
        return pre
    b3, sb3 = q.contiguous().view(batch, K, N), s.contiguous().view(batch, K // bs, N)
    return mx_gemm._pack(b3, sb3, fid, bs, batch, N, K, (K * N, 1, N), (sb3.stride(0), 1, sb3.stride(1)), check=False)


def same(a, b):
    a, b = a.contiguous(), b.contiguous()
    bits = torch.int16 if a.dtype == torch.bfloat16 else (torch.int32 if a.dtype == torch.float32 else a.dtype)
    return a.shape == b.shape and torch.equal(a.view(bits), b.view(bits))


def quantize_row(label, shape, dtype, fmt, bs, ax, pow2, scale_fmt=None, operand=False, view=None, last_axis=True):
    from quantized_training.fake_quantize import get_quantization_map
    from quantized_training.quantizer.quantizer import get_quant_min_max
    qmap = get_quantization_map(fmt, "cuda")
    smap = get_quantization_map(scale_fmt, "cuda") if scale_fmt else None
    qmax = float(get_quant_min_max(fmt)[1])
    pool, numel = make_pool(shape, dtype, view)

    def call(x, axes):
        s, q = torch.ops.quantized_ops.quantize_mx(x, qmap, axes, bs, qmax, pow2, smap, None)
        return (s, q) + (tuple(matmul_operand(q, s, bs)) if operand else ())

    routes = {"kernel": lambda x: call(x, [ax]), "parent": as_parent(lambda x: call(x, [ax]))}
    if last_axis:
        routes["last-axis"] = lambda x: torch.ops.quantized_ops.quantize_mx(x, qmap, [-1], bs, qmax, pow2, smap, None)
    got, want = routes["kernel"](pool[0]), routes["parent"](pool[0])
    assert all(same(g.reshape(w.shape), w) for g, w in zip(got, want)), f"{label}: the kernel and the parent route disagree"
    item = 2 if dtype == torch.bfloat16 else 4
    nbytes = 2 * numel * item + (numel // bs) * item
    if operand:
        from quantized_training import mx_gemm
        nbytes += numel * mx_gemm._BITS[mx_gemm.FMT_ID[fmt]] // 8 + numel // 32
    return label, nbytes, measure(routes, pool)


def fake_quant_row(label, shape, spec, pow2):
    import quantized_training as qt
    kw = asdict(qt.QuantizationSpec.from_str(spec))
    m = qt.FusedAmaxObsFakeQuantize(**kw, force_scale_power_of_two=pow2, device="cuda")
    ref = qt.FusedAmaxObsFakeQuantize(**kw, force_scale_power_of_two=pow2, device="cuda")
    pool, numel = make_pool(shape, torch.bfloat16)
    routes = {"kernel": lambda x: m(x), "parent": as_parent(lambda x: ref(x))}
    y, yp = routes["kernel"](pool[0]), routes["parent"](pool[0])
    assert same(y, yp) and same(m.scale, ref.scale), f"{label}: the kernel and the parent route disagree"
    nbytes = 2 * numel * 2 + (numel // m.block_size) * 2
    return label, nbytes, measure(routes, pool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_strided.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_mx_strided.py measures on the GPU and there is none: nothing measured")
    torch.manual_seed(0)
    bf16, f32 = torch.bfloat16, torch.float32
    rows = []
    with torch.no_grad():
        rows.append(quantize_row("value [1,32,1024,128] bf16 fp8_e4m3 bs=32 ax=-2 pow2: quantize_mx + matmul operand", (1, 32, 1024, 128), bf16,
                                 "fp8_e4m3", 32, -2, True, operand=True))
        rows.append(fake_quant_row("value [1,32,1024,128] bf16 fp8_e4m3 bs=32 ax=-2 pow2: fake-quant module", (1, 32, 1024, 128),
                                   "fp8_e4m3,qs=microscaling,bs=32,ax=-2", True))
        rows.append(quantize_row("[16,12,384,64] bf16 fp4_e2m1 bs=32 ax=-2 pow2: quantize_mx + matmul operand", (16, 12, 384, 64), bf16,
                                 "fp4_e2m1", 32, -2, True, operand=True))
        rows.append(quantize_row("[1024,4096] fp32 fp8_e4m3 bs=32 ax=0 amax/qmax scale=fp8_e4m3: quantize_mx", (1024, 4096), f32,
                                 "fp8_e4m3", 32, 0, False, scale_fmt="fp8_e4m3"))
        rows.append(quantize_row("key [1,32,1024,128]^T bf16 fp8_e4m3 bs=32 ax=-2 pow2: quantize_mx + matmul operand", (1, 32, 1024, 128), bf16,
                                 "fp8_e4m3", 32, -2, True, operand=True, view=lambda t: t.transpose(-1, -2), last_axis=False))
    lines = [f"# tools/exp_mx_strided.py on {torch.cuda.get_device_name(0)}; {REPEATS} repeats per route, routes alternating, "
             f"{WINDOW_MS:.0f} ms windows between device events",
             "# time per call in microseconds: min / median / max; TB/s = algorithmic bytes / median",
             f"{'row':<88} {'route':<10} {'min':>9} {'median':>9} {'max':>9} {'TB/s':>6}  verdict"]
    for label, nbytes, res in rows:
        parent_min = res["parent"][0]
        for name, t in res.items():
            med = statistics.median(t)
            verdict = ""
            if name == "kernel":
                verdict = "clears the bar" if t[-1] < parent_min else "DOES NOT clear the bar"
                verdict += f" ({statistics.median(res['parent']) / med:.1f}x the parent route)"
            lines.append(f"{label:<88} {name:<10} {t[0] * 1e3:9.1f} {med * 1e3:9.1f} {t[-1] * 1e3:9.1f} {nbytes / (med * 1e-3) / 1e12:6.2f}  {verdict}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
