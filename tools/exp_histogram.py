"""record_histogram on the device: the reference's torch composite (QT_HISTOGRAM=0) against the HIP route (default), both in one process.

Per row, bf16: the MODULE call of a FusedAmaxObsFakeQuantize with record_histogram (histogram + fake-quant: composite + qt_fake_quant_bf16
against the one launch of qt_fake_quant_hist_bf16), the same module without the flag (what the fake-quant pass alone costs), and the
HISTOGRAM ALONE (the composite's two lines against qt_exp_histogram_bf16).  Rows: a [1024, 4096] activation, a [11008, 4096] weight, a
[2048, 768] gradient with E5M2, [1, 32, 1024, 128], all normal random; and the [11008, 4096] tensor all-equal -- every lane of every
LDS add on one bin, the contention worst case, to be read against the random row of the same size.

Method: operands rotate over a pool larger than the 256 MB Infinity Cache; warm-up, then REPEATS rounds in which the routes alternate,
a round timing ITERS passes over the pool between two events; median [min, max] in us per call, for eager calls and for hipGraph replays
(one graph per route holding one call per pool tensor).  TB/s is the bytes of x over the histogram-alone time, against the chip's
6.29 TB/s copy figure.  The bar: native is the default only where its median beats the composite's by more than the composite's own
min - max spread, in both modes.  The table is committed as profiles/exp_histogram.txt.

    timeout -k 10 900 python tools/exp_histogram.py [--iters 3] [--repeats 7] [--out profiles/exp_histogram.txt]
"""
import argparse
import os
import statistics
import sys
from dataclasses import asdict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
import quantized_training as qt  # noqa: E402
from quantized_training import histogram  # noqa: E402

DEV = torch.device("cuda:0")
POOL_BYTES = 320e6
COPY_TBS = 6.29
ROWS = [("activation [1024, 4096]", (1024, 4096), "e4m3", "normal"),
        ("weight [11008, 4096]", (11008, 4096), "e4m3", "normal"),
        ("gradient [2048, 768] e5m2", (2048, 768), "e5m2", "normal"),
        ("[1, 32, 1024, 128]", (1, 32, 1024, 128), "e4m3", "normal"),
        ("weight [11008, 4096] all-equal", (11008, 4096), "e4m3", "equal")]


def module(spec, flag):
    kw = asdict(qt.QuantizationSpec.from_str(spec))
    m = qt.FusedAmaxObsFakeQuantize(**kw, record_histogram=flag, device=DEV)
    m._move_to(DEV)
    return m


def routed(native, fn):
    def call(x):
        if native:
            os.environ.pop("QT_HISTOGRAM", None)
        else:
            os.environ["QT_HISTOGRAM"] = "0"
        return fn(x)
    return call


def time_rounds(fns, pool, iters, repeats, captured):
    """{name: (median, min, max)} us per call."""
    runs = {}
    for name, fn in fns.items():
        if captured:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            try:
                with torch.cuda.stream(s), torch.no_grad():
                    for x in pool[:2]:
                        fn(x)                                       # allocations and scratch exist before the capture
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=s):
                        for x in pool:
                            fn(x)
                runs[name] = g.replay
            except RuntimeError as e:                               # a route that cannot be captured is reported, not timed
                print(f"  ({name}: capture failed: {str(e).splitlines()[0]})", flush=True)
            torch.cuda.current_stream().wait_stream(s)
        else:
            def eager(fn=fn):
                with torch.no_grad():
                    for x in pool:
                        fn(x)
            runs[name] = eager
    for run in runs.values():
        for _ in range(2):
            run()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(repeats):
        for name, run in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                run()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / (iters * len(pool)))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = [f"record_histogram: torch composite (QT_HISTOGRAM=0) against the HIP route; {torch.cuda.get_device_name(0)}; us per call, "
             f"median [min, max] of {args.repeats} rounds x {args.iters} passes over a rotating pool > {POOL_BYTES / 1e6:.0f} MB",
             f"TB/s: bytes of x over the histogram-alone time ({COPY_TBS} TB/s = the chip's copy figure)", ""]

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    verdicts = []
    for name, shape, spec, data in ROWS:
        n = 1
        for d in shape:
            n *= d
        count = max(2, min(48, int(POOL_BYTES // (2 * n)) + 1))
        torch.manual_seed(0)
        pool = [(torch.randn(shape, device=DEV) if data == "normal" else torch.full(shape, 0.75, device=DEV)).bfloat16() for _ in range(count)]
        m_hist, m_plain = module(spec, True), module(spec, False)
        hist = torch.zeros(254, device=DEV)
        fns = {"module composite": routed(False, m_hist), "module native": routed(True, m_hist), "module, no histogram": routed(True, m_plain),
               "histogram composite": routed(False, lambda x: histogram.record(x, hist)),
               "histogram native": routed(True, lambda x: histogram.record(x, hist))}
        # the routes are the ones named
        histogram.reset_stats()
        with torch.no_grad():
            fns["module native"](pool[0]); fns["histogram native"](pool[0]); fns["module composite"](pool[0]); fns["histogram composite"](pool[0])
        assert histogram.STATS == {"histogram_native": 1, "histogram_fused": 1, "histogram_composite": 2}, histogram.STATS
        emit(f"== {name}, {spec}, {data}: {n} elements, pool of {count}")
        for captured in (False, True):
            mode = "hipGraph replay" if captured else "eager"
            r = time_rounds(fns, pool, args.iters, args.repeats, captured)
            for k in fns:
                if k not in r:
                    emit(f"  {mode:16s} {k:22s} not capturable")
            if len(r) < len(fns):
                verdicts.extend((name, mode, what, False, 0.0) for what in ("module", "histogram"))
                continue
            for k, (med, lo, hi) in r.items():
                extra = f"   {2 * n / med / 1e6:6.2f} TB/s of x ({2 * n / med / 1e6 / COPY_TBS * 100:4.1f} % of copy)" if k.startswith("histogram") else ""
                emit(f"  {mode:16s} {k:22s} {med:9.1f} [{lo:9.1f}, {hi:9.1f}]{extra}")
            for what in ("module", "histogram"):
                c, nat = r[f"{what} composite"], r[f"{what} native"]
                ok = nat[0] < c[0] - (c[2] - c[1])
                verdicts.append((name, mode, what, ok, c[0] / nat[0]))
                emit(f"  {mode:16s} {what:10s} native / composite: {c[0] / nat[0]:6.2f} x   bar (median beats the composite's by more than its spread): "
                     f"{'cleared' if ok else 'NOT cleared'}")
        emit()
    emit(f"bar cleared on {sum(v[3] for v in verdicts)} of {len(verdicts)} (row, mode, what) entries"
         + ("" if all(v[3] for v in verdicts) else "; NOT cleared: " + "; ".join(f"{v[0]} / {v[1]} / {v[2]}" for v in verdicts if not v[3])))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
