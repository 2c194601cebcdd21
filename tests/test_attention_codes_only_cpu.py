"""The codes-only decision of the FP8 attention core (attention_route.attention_output_plan): the kernel may leave the bf16 values unwritten only
while nobody but the output projection's own code path can see them."""
import pytest
import torch

import quantized_training as qt
from quantized_training import attention_route, handover

IDS = torch.randint(3, 97, (2, 16), generator=torch.Generator().manual_seed(0))


def _planned_llama():
    pytest.importorskip("transformers")
    from transformers import LlamaConfig, LlamaModel
    torch.manual_seed(0)
    model = LlamaModel(LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                                   vocab_size=97, max_position_embeddings=32, attn_implementation="eager"))
    model = model.eval().bfloat16()
    qt.quantize(model, qt.add_qspec_args().parse_args(["--activation", "e4m3", "--weight", "e4m3", "--bf16"]))
    with torch.no_grad():
        model(IDS)                                                           # the first call creates the fake-quantizers
    return model.layers[0].self_attn


@pytest.mark.parametrize("hooked", ["nothing", "o_proj's input fake-quantizer", "the attention module"])
def test_attention_codes_only_declines_when_someone_can_see_the_values(hooked, monkeypatch):
    attn = _planned_llama()
    fq_o = attn.o_proj.activation_pre_process["0"]
    target = {"nothing": None, "o_proj's input fake-quantizer": fq_o, "the attention module": attn}[hooked]
    if target is not None:
        target.register_forward_hook(lambda m, a, out: None)
    with torch.no_grad():
        got_fq, codes_only = attention_route.attention_output_plan(attn)
        assert got_fq is fq_o                                                # the epilogue still applies the fake-quantizer: values AND codes
        assert codes_only is (hooked == "nothing")
        monkeypatch.setenv("QT_CODES_ONLY", "0")
        assert attention_route.attention_output_plan(attn) == (fq_o, False)
    assert attention_route.attention_output_plan(attn) == (fq_o, False)                # gradients on: somebody will read the values


def test_view_of_a_codes_only_result_goes_through_the_consumer_undecoded(monkeypatch):
    """What the output projection's hook does with HF's reshaped view of a codes-only attention result: with `_qt_lazy_ok` (the Linear
    multiplies the codes) the view goes through lazy, carrying the codes, and is decoded exactly on demand; without it the values are
    decoded there and then.  QT_LAZY_POISON=1 (the suite's setting) makes an undecoded read NaN."""
    monkeypatch.setenv("QT_LAZY_POISON", "1")
    spec = qt.QuantizationSpec.from_str("e4m3")
    from dataclasses import asdict
    vals = torch.randn(2, 8, 4, 16).bfloat16()
    for lazy_ok in (True, False):
        fq = qt.FusedAmaxObsFakeQuantize(**asdict(spec))
        assert fq.producer_fusable()
        codes = vals.to(torch.float8_e4m3fn)
        want = codes.to(torch.bfloat16).reshape(2, 8, 64)
        out = handover.unwritten(vals.shape, torch.bfloat16, vals.device)
        handover.stamp(out, fq, codes, lazy=True)
        fq.expect_prequantized(out, codes)
        if lazy_ok:
            fq.__dict__["_qt_lazy_ok"] = True
        view = out.reshape(2, 8, 64)
        assert torch.isnan(view).all()
        got = fq(view)
        assert handover.is_lazy(got) is lazy_ok
        if lazy_ok:
            assert torch.equal(handover.codes(got).view(torch.uint8), codes.view(torch.uint8).reshape(2, 8, 64))
            assert torch.isnan(got).all()
            handover.materialize(got)
        assert torch.equal(got, want)
