"""Times the any-key-count FP8 attention core (qt_value_codes_t_ragged + qt_attention_fp8_ragged, with the two code passes over q and k that
feed it) against the route the same call takes without it, both through the module path's own entry (quantizable_attention_forward on the
self-attention block of a quantized stateless-E4M3 BERT layer, q / k / v as transpose_for_scores leaves them): QT_FUSED_ATTENTION=1
against the switch unset with attention_route._FP8_RAGGED_TABLE emptied for this process -- the route of the commit before the kernel: the
two-pass bf16 core behind three fake-quant passes where C % 4 == 0 at head_dim 64, the library / torch chain elsewhere.  (The kernel
route returns fq_o(result), the other the result: they differ by at most half a step of the output projection's format.)  ONE process, the two routes
alternating, eager and replayed from a captured graph, with a right-padding mask (lengths spread over 40 .. 100 % of S) and without a
mask.  Prints medians with min-max; the lines are what profiles/attention_fp8_ragged.txt holds and what _FP8_RAGGED_TABLE is read from (a
class is taken when the kernel's median beats the parent route's by more than that route's min-max spread in all four rows).
python tools/exp_attention_fp8_ragged.py [OUT.txt]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-training_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import quantized_training as qt  # noqa: E402
from quantized_training import attention_route  # noqa: E402
from quantized_training.modules.quantizable.attention import quantizable_attention_forward  # noqa: E402
from exp_attention_fp8_long import DEV, SAMPLES, alternating, captured, fmt_us  # noqa: E402

# (B, H, S, D): ViT-base; GLUE batches padded to their longest sample; SQuAD short of a block; one head_dim 128 shape
SHAPES = ((16, 12, 197, 64), (32, 12, 77, 64), (32, 12, 136, 64), (32, 12, 200, 64), (16, 12, 300, 64), (16, 16, 376, 64), (4, 32, 200, 128))
ITERS = 100                 # calls per sample: about ten milliseconds of work


def attention_block(D):
    """The self-attention block of a quantized one-layer BERT with heads of D, its fake-quantizers created by a first forward."""
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    m = BertModel(BertConfig(hidden_size=2 * D, num_hidden_layers=1, num_attention_heads=2, intermediate_size=4 * D, vocab_size=300,
                             max_position_embeddings=64)).eval().bfloat16().to(DEV)
    qt.quantize(m, qt.add_qspec_args().parse_args(["--activation", "e4m3", "--weight", "e4m3", "--bf16"]))
    with torch.no_grad():
        m(torch.randint(3, 300, (2, 24), device=DEV))
    return m, m.encoder.layer[0].attention.self


def main():
    out_file = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    attention_route._FP8_RAGGED_TABLE.clear()               # the unset route is then the one without the kernel
    say(f"# tools/exp_attention_fp8_ragged.py on {torch.cuda.get_device_name(0)}: medians of {SAMPLES} samples (min-max), the two routes alternating")
    blocks = {}
    for (B, H, S, D) in SHAPES:
        if D not in blocks:
            blocks[D] = attention_block(D)
        attn = blocks[D][1]
        q, k, v = (torch.randn(B, S, H, D, device=DEV).bfloat16().transpose(1, 2) for _ in range(3))      # as transpose_for_scores leaves them
        lengths = torch.linspace(0.4 * S, S, B).round().long()
        pad = torch.zeros(B, 1, 1, S, dtype=torch.bfloat16, device=DEV)
        for i, n in enumerate(lengths.tolist()):
            pad[i, :, :, n:] = torch.finfo(torch.bfloat16).min
        for masked in (True, False):
            mask = pad if masked else None

            def route(switch):
                def call():
                    os.environ.pop("QT_FUSED_ATTENTION", None)
                    if switch:
                        os.environ["QT_FUSED_ATTENTION"] = switch
                    with torch.no_grad():
                        return quantizable_attention_forward(attn, q, k, v, mask)[0]
                return call

            parent, kernel = route(None), route("1")
            tag = f"B {B} H {H} S {S} D {D} {'padding' if masked else 'unmasked'}"
            attention_route.ATTENTION_ROUTES.clear()
            a, b = parent().float(), kernel().float()
            took = attention_route.ATTENTION_ROUTES.get(f"attention:{B}x{H}x{S}x{S}x{D}")
            say(f"# {tag}: the switch's route is {took}; max |kernel - parent| {(a - b).abs().max().item():.4f} at max |parent| {a.abs().max().item():.3f}")
            tp, tk = alternating(parent, kernel, ITERS)
            say(f"{tag}  eager  parent {fmt_us(tp)}  kernel {fmt_us(tk)}")
            try:
                gp, gk = captured(parent), captured(kernel)
                tp, tk = alternating(gp, gk, ITERS)
                say(f"{tag}  graph  parent {fmt_us(tp)}  kernel {fmt_us(tk)}")
            except Exception as e:  # noqa: BLE001 -- a route that cannot be captured is a result, not a crash of the session
                say(f"{tag}  graph  not captured: {type(e).__name__}: {str(e)[:120]}")
    os.environ.pop("QT_FUSED_ATTENTION", None)
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
