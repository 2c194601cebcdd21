"""Times the streaming FP8 attention core (qt_value_codes_t + qt_attention_fp8_long) against the chain that serves key counts beyond 1024
today -- Q.K^T as a batched library FP8 GEMM, the score pass (qt_softmax_fq_bf16_fp8), the value pass (qt_fake_quant_rows_bf16_fp8) and
P.V as a batched library FP8 GEMM -- both in ONE process, alternating, eager and replayed from a captured graph.  Prints medians with
min-max, and the chain's peak temporary memory; the lines are what profiles/attention_fp8_long.txt holds and what
attention_route._FP8_LONG_TABLE is read from (a class is taken when the kernel's median beats the chain's by more than the chain's
min-max spread in both modes).   python tools/exp_attention_fp8_long.py [OUT.txt]"""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
from quantized_training import _native  # noqa: E402
from quantized_training.fused import lt_fp8_gemm  # noqa: E402

L = _native.lib()
DEV = torch.device("cuda:0")
SHAPES = ((1, 32, 2048, True, 128), (1, 32, 4096, True, 128), (1, 32, 8192, True, 128), (4, 12, 2048, False, 64))
SAMPLES = 9


def st():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def sample(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def alternating(a, b, iters):
    """SAMPLES timings of each, a and b taking turns."""
    for _ in range(2):
        a(); b()
    ta, tb = [], []
    for _ in range(SAMPLES):
        ta.append(sample(a, iters))
        tb.append(sample(b, iters))
    return ta, tb


def fmt_us(ts):
    return f"{statistics.median(ts):8.1f} ({min(ts):.1f}-{max(ts):.1f}) us"


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
        fn()
    torch.cuda.synchronize()
    return g.replay


def main():
    out_file = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    fmt = _native.format_for("e4m3")
    say(f"# tools/exp_attention_fp8_long.py on {torch.cuda.get_device_name(0)}: medians of {SAMPLES} samples (min-max), the two routes alternating")
    for (B, H, S, causal, D) in SHAPES:
        q8 = torch.randn(B, H, S, D, device=DEV).to(torch.float8_e4m3fn)
        k8 = torch.randn(B, H, S, D, device=DEV).to(torch.float8_e4m3fn)
        v = torch.randn(B, S, H, D, device=DEV).bfloat16().transpose(1, 2)           # as the v projection leaves it
        mask = torch.full((S, S), torch.finfo(torch.bfloat16).min, device=DEV).triu(1).bfloat16()[None, None] if causal else None
        mp, msq = (mask.data_ptr(), S) if causal else (None, 0)
        rl = None
        if causal:
            rl = torch.empty(S + 1, dtype=torch.int32, device=DEV)
            _native.check(L.qt_mask_row_live_checked(mp, S, S, S, rl.data_ptr(), rl.data_ptr() + 4 * S, st()), "live")
        vt8 = torch.empty(B, H, D, S, dtype=torch.uint8, device=DEV)
        out = torch.empty(B, S, H, D, dtype=torch.bfloat16, device=DEV)
        v8 = torch.empty(B, H, S, D, dtype=torch.uint8, device=DEV)
        scaling = D ** -0.5

        def kernel():
            _native.check(L.qt_value_codes_t(v.data_ptr(), vt8.data_ptr(), B, H, S, D, v.stride(0), v.stride(1), v.stride(2), ctypes.byref(fmt), st()), "vt")
            _native.check(L.qt_attention_fp8_long(q8.data_ptr(), k8.data_ptr(), vt8.data_ptr(), 0, mp, 0, 0, msq, rl.data_ptr() if causal else None, 0, 0,
                                                  1 if causal else 0, 0, rl.data_ptr() + 4 * S if causal else None, out.data_ptr(), None, None, B, H, S, S, D,
                                                  scaling, st()), "attn")

        def chain():
            sc = lt_fp8_gemm(q8.view(B * H, S, D), k8.view(B * H, S, D))                                  # [BH, S, S] bf16
            p8 = torch.empty(B, H, S, S, dtype=torch.uint8, device=DEV)
            _native.check(L.qt_softmax_fq_bf16_fp8(sc.data_ptr(), mp, None, p8.data_ptr(), B, H, S, S, 0, 0, msq, scaling, ctypes.byref(fmt), st()), "softmax")
            _native.check(L.qt_fake_quant_rows_bf16_fp8(v.data_ptr(), None, v8.data_ptr(), B, H, S, D, v.stride(0), v.stride(1), v.stride(2),
                                                        ctypes.byref(fmt), st()), "vpass")
            return lt_fp8_gemm(p8.view(torch.float8_e4m3fn).view(B * H, S, S), v8.view(torch.float8_e4m3fn).view(B * H, S, D), None, b_is_kn=True)

        tag = f"B {B} H {H} S {S} D {D} {'causal' if causal else 'unmasked'}"
        if S > 4096 or chain() is None:               # (the score pass takes at most 4096 columns)
            say(f"{tag}: the chain does not take this shape; kernel alone {fmt_us([sample(kernel, 3) for _ in range(SAMPLES)])}")
            continue
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        chain()
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        iters = 5 if S <= 2048 else 3
        tc, tk = alternating(chain, kernel, iters)
        say(f"{tag}  eager  chain {fmt_us(tc)}  kernel {fmt_us(tk)}  chain peak temporaries {peak:.0f} MiB")
        try:
            gc, gk = captured(chain), captured(kernel)
            tc, tk = alternating(gc, gk, iters)
            say(f"{tag}  graph  chain {fmt_us(tc)}  kernel {fmt_us(tk)}")
        except Exception as e:  # noqa: BLE001 -- a route that cannot be captured is a result, not a crash of the session
            say(f"{tag}  graph  not captured: {type(e).__name__}: {str(e)[:120]}")
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
