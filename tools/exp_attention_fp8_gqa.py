"""Times the grouped-query FP8 attention route (the code passes over q and the UNREPEATED k, qt_value_codes_t with H = Hkv,
qt_attention_fp8_gqa) against the route the same call takes without it, both through the module path's own entry
(quantizable_attention_forward on the attention block of a quantized stateless-E4M3 LLaMA layer with grouped heads, q / k / v as the
projections leave them): QT_FUSED_ATTENTION=1 against the switch unset with attention_route._FP8_GQA_TABLE emptied for this process --
the route of the commit before the kernel: _repeat_kv's copies of K and V, the code passes over G times the data, then qt_attention_fp8
(up to 1024 keys), qt_attention_fp8_long where _FP8_LONG_TABLE lists the repeated shape, else the library chain.  ONE process, the two
routes alternating, eager and replayed from a captured graph, with the causal mask and without a mask.  Prints medians with min-max and
both routes' peak temporary bytes; the lines are what profiles/attention_fp8_gqa.txt holds and what _FP8_GQA_TABLE is read from (a class
is taken when the kernel route's median beats the parent route's by more than that route's min-max spread in all four rows).
python tools/exp_attention_fp8_gqa.py [OUT.txt]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import quantized_training as qt  # noqa: E402
from quantized_training import attention_route, handover  # noqa: E402
from quantized_training.modules.quantizable.attention import _causal_mask, quantizable_attention_forward  # noqa: E402
from exp_attention_fp8_long import DEV, SAMPLES, alternating, captured, fmt_us  # noqa: E402

# (B, H, Hkv, S, D): Llama-3-8B / Mistral-7B; Llama-3.2-1B; TinyLlama; Llama-2-70B
SHAPES = ((1, 32, 8, 1024, 128), (1, 32, 8, 2048, 128), (1, 32, 8, 4096, 128), (1, 32, 8, 2048, 64), (1, 32, 4, 2048, 64), (1, 64, 8, 4096, 128))


def attention_block(G, D):
    """The attention block of a quantized one-layer LLaMA with G query heads of D over one kv head, its fake-quantizers created by a first
    forward.  (The entry is handed q / k / v of any head count; of the block it reads the group size, the hooks and the projection.)"""
    from transformers import LlamaConfig, LlamaModel
    torch.manual_seed(0)
    m = LlamaModel(LlamaConfig(hidden_size=G * D, intermediate_size=2 * G * D, num_hidden_layers=1, num_attention_heads=G, num_key_value_heads=1,
                               vocab_size=320, max_position_embeddings=64)).eval().bfloat16().to(DEV)
    qt.quantize(m, qt.add_qspec_args().parse_args(["--activation", "e4m3", "--weight", "e4m3", "--bf16"]))
    with torch.no_grad():
        m(torch.randint(3, 320, (1, 24), device=DEV), use_cache=False)
    return m, m.layers[0].self_attn


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    del out
    return peak


def main():
    out_file = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    attention_route._FP8_GQA_TABLE.clear()                  # the unset route is then the one without the kernel
    say(f"# tools/exp_attention_fp8_gqa.py on {torch.cuda.get_device_name(0)}: medians of {SAMPLES} samples (min-max), the two routes alternating")
    blocks = {}
    for (B, H, Hkv, S, D) in SHAPES:
        G = H // Hkv
        if (G, D) not in blocks:
            blocks[G, D] = attention_block(G, D)
        attn = blocks[G, D][1]
        q = torch.randn(B, S, H, D, device=DEV).bfloat16().transpose(1, 2)           # as the projections leave them
        k, v = (torch.randn(B, S, Hkv, D, device=DEV).bfloat16().transpose(1, 2) for _ in range(2))
        iters = max(3, 40 * 1024 // S)
        for masked in (True, False):
            mask = _causal_mask(S, S, torch.bfloat16, DEV) if masked else None

            def route(switch):
                def call():
                    os.environ.pop("QT_FUSED_ATTENTION", None)
                    if switch:
                        os.environ["QT_FUSED_ATTENTION"] = switch
                    with torch.no_grad():
                        return quantizable_attention_forward(attn, q, k, v, mask, is_causal=False)[0]
                return call

            parent, kernel = route(None), route("1")
            tag = f"B {B} H {H} Hkv {Hkv} S {S} D {D} {'causal' if masked else 'unmasked'}"
            attention_route.ATTENTION_ROUTES.clear()
            a, b = parent(), kernel()
            took = dict(attention_route.ATTENTION_ROUTES)
            handover.materialize(a)
            handover.materialize(b)
            a, b = a.float(), b.float()
            say(f"# {tag}: routes {took}; max |kernel - parent| {(a - b).abs().max().item():.4f} at max |parent| {a.abs().max().item():.3f}; "
                f"peak temporaries parent {peak_mib(parent):.1f} MiB, kernel {peak_mib(kernel):.1f} MiB")
            tp, tk = alternating(parent, kernel, iters)
            say(f"{tag}  eager  parent {fmt_us(tp)}  kernel {fmt_us(tk)}")
            try:
                gp, gk = captured(parent), captured(kernel)
                tp, tk = alternating(gp, gk, iters)
                say(f"{tag}  graph  parent {fmt_us(tp)}  kernel {fmt_us(tk)}")
            except Exception as e:  # noqa: BLE001 -- a route that cannot be captured is a result, not a crash of the session
                say(f"{tag}  graph  not captured: {type(e).__name__}: {str(e)[:120]}")
    os.environ.pop("QT_FUSED_ATTENTION", None)
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
