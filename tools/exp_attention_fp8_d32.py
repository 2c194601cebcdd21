"""Times the head_dim 32 FP8 attention core (qt_value_codes_t_d32 + qt_attention_fp8_d32) against the chain that serves MobileBERT's
attention today -- Q.K^T as a batched library FP8 GEMM, the score pass (qt_softmax_fq_bf16_fp8), the value pass
(qt_fake_quant_rows_bf16_fp8) and P.V as a batched library FP8 GEMM -- both in ONE process, alternating, eager and replayed from a
captured graph, with a right-padding mask (lengths spread over 40 .. 100 % of S) and without a mask.  Prints medians with min-max; the
lines are what profiles/attention_fp8_d32.txt holds and what attention_route._FP8_D32_TABLE is read from (a class is taken when the
kernel's median beats the chain's by more than the chain's min-max spread in all four rows).
python tools/exp_attention_fp8_d32.py [OUT.txt]"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from quantized_training import _native  # noqa: E402
from quantized_training.fused import lt_fp8_gemm  # noqa: E402
from exp_attention_fp8_long import DEV, L, SAMPLES, alternating, captured, fmt_us, st  # noqa: E402

SHAPES = ((16, 4, 384), (32, 4, 128), (16, 4, 512))       # the SQuAD recipe; short and full-length batches
D = 32
ITERS = 200                 # launches per sample: tens of milliseconds of work


def main():
    out_file = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    fmt = _native.format_for("e4m3")
    say(f"# tools/exp_attention_fp8_d32.py on {torch.cuda.get_device_name(0)}: medians of {SAMPLES} samples (min-max), the two routes alternating")
    for (B, H, S) in SHAPES:
        q8 = torch.randn(B, H, S, D, device=DEV).to(torch.float8_e4m3fn)
        k8 = torch.randn(B, H, S, D, device=DEV).to(torch.float8_e4m3fn)
        v = torch.randn(B, S, H, D, device=DEV).bfloat16().transpose(1, 2)           # as the v projection leaves it
        vt8 = torch.empty(B, H, D, S, dtype=torch.uint8, device=DEV)
        out = torch.empty(B, S, H, D, dtype=torch.bfloat16, device=DEV)
        v8 = torch.empty(B, H, S, D, dtype=torch.uint8, device=DEV)
        scaling = D ** -0.5
        lengths = torch.linspace(0.4 * S, S, B).round().long()
        pad = torch.zeros(B, 1, 1, S, dtype=torch.bfloat16, device=DEV)
        for i, n in enumerate(lengths.tolist()):
            pad[i, :, :, n:] = torch.finfo(torch.bfloat16).min
        rl = torch.empty(B + 1, dtype=torch.int32, device=DEV)
        _native.check(L.qt_mask_row_live_checked(pad.data_ptr(), B, S, S, rl.data_ptr(), rl.data_ptr() + 4 * B, st()), "live")
        for masked in (True, False):
            mp, msb = (pad.data_ptr(), S) if masked else (None, 0)
            live = (rl.data_ptr(), 1, 0, 0) if masked else (None, 0, 0, 0)
            flag = rl.data_ptr() + 4 * B if masked else None

            def kernel():
                _native.check(L.qt_value_codes_t_d32(v.data_ptr(), vt8.data_ptr(), B, H, S, v.stride(0), v.stride(1), v.stride(2), ctypes.byref(fmt), st()), "vt")
                _native.check(L.qt_attention_fp8_d32(q8.data_ptr(), k8.data_ptr(), vt8.data_ptr(), 0, mp, msb, 0, 0, *live, 0, flag, out.data_ptr(), None,
                                                     None, B, H, S, S, D, scaling, st()), "attn")

            def chain():
                sc = lt_fp8_gemm(q8.view(B * H, S, D), k8.view(B * H, S, D))                                  # [BH, S, S] bf16
                p8 = torch.empty(B, H, S, S, dtype=torch.uint8, device=DEV)
                _native.check(L.qt_softmax_fq_bf16_fp8(sc.data_ptr(), mp, None, p8.data_ptr(), B, H, S, S, msb, 0, 0, scaling, ctypes.byref(fmt), st()), "softmax")
                _native.check(L.qt_fake_quant_rows_bf16_fp8(v.data_ptr(), None, v8.data_ptr(), B, H, S, D, v.stride(0), v.stride(1), v.stride(2),
                                                            ctypes.byref(fmt), st()), "vpass")
                return lt_fp8_gemm(p8.view(torch.float8_e4m3fn).view(B * H, S, S), v8.view(torch.float8_e4m3fn).view(B * H, S, D), None, b_is_kn=True)

            tag = f"B {B} H {H} S {S} D {D} {'padding' if masked else 'unmasked'}"
            if chain() is None:
                say(f"{tag}: the chain does not take this shape; kernel alone {fmt_us([t for t in alternating(kernel, kernel, ITERS)[0]])}")
                continue
            tc, tk = alternating(chain, kernel, ITERS)
            say(f"{tag}  eager  chain {fmt_us(tc)}  kernel {fmt_us(tk)}")
            try:
                gc, gk = captured(chain), captured(kernel)
                tc, tk = alternating(gc, gk, ITERS)
                say(f"{tag}  graph  chain {fmt_us(tc)}  kernel {fmt_us(tk)}")
            except Exception as e:  # noqa: BLE001 -- a route that cannot be captured is a result, not a crash of the session
                say(f"{tag}  graph  not captured: {type(e).__name__}: {str(e)[:120]}")
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
