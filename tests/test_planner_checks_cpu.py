"""quantized_training/planner_checks.py: each predicate against each of nn.Module's four hook kinds, the holder look-ups against holders
of 0..3 fake-quantizers, plain_per_tensor against the fake-quantizers it must refuse -- and what the planners answer on quantized
tiny BERT / LLaMA models when a user hooks a norm, the softmax or a consumer's fake-quantizer."""
from dataclasses import asdict

import pytest
import torch
from torch import nn

import quantized_training as qt
from quantized_training import attention_route, fused, model_fusions as mf, planner_checks as pc

KINDS = ["forward_pre", "forward", "backward_pre", "backward"]


def _hooked(*kinds):
    mod = nn.Linear(4, 4)
    for kind in kinds:
        {"forward_pre": lambda: mod.register_forward_pre_hook(lambda m, a: None),
         "forward": lambda: mod.register_forward_hook(lambda m, a, o: None),
         "backward_pre": lambda: mod.register_full_backward_pre_hook(lambda m, g: None),
         "backward": lambda: mod.register_full_backward_hook(lambda m, gi, go: None)}[kind]()
    return mod


# predicate -> (no hook, forward_pre, forward, backward_pre, backward), one hook at a time
PREDICATES = {
    "no_hooks": (pc.no_hooks, [True, False, False, False, False]),
    "no_forward_hooks": (pc.no_forward_hooks, [True, False, False, True, True]),
    "no_output_hook": (pc.no_output_hook, [True, True, False, True, True]),
    "only_pre_hooks": (pc.only_pre_hooks, [True, True, False, False, False]),
    "quantize_hooks_only": (pc.quantize_hooks_only, [False, True, False, False, False]),
    "quantize_hooks_only, none registered": (lambda m: pc.quantize_hooks_only(m, 0), [True, False, False, True, True]),
    "quantize_hooks_only, training": (lambda m: pc.quantize_hooks_only(m, 1, backward_pre=1), [False, False, False, False, False]),
    "hook_counts, at most one pre-hook": (lambda m: pc.hook_counts(m, forward_pre=(0, 1)), [True, True, True, True, True]),
    "hook_counts, one backward hook": (lambda m: pc.hook_counts(m, backward=1), [False, False, False, False, True]),
}


@pytest.mark.parametrize("name", sorted(PREDICATES))
def test_predicate_against_each_hook_kind(name):
    check, expected = PREDICATES[name]
    got = [check(_hooked())] + [check(_hooked(kind)) for kind in KINDS]
    assert got == expected and all(type(g) is bool for g in got)


def test_predicates_on_hook_combinations():
    both = _hooked("forward_pre", "backward_pre")
    assert pc.quantize_hooks_only(both) and pc.quantize_hooks_only(both, 1, backward_pre=1) and pc.only_pre_hooks(_hooked("forward_pre", "forward_pre"))
    assert not pc.quantize_hooks_only(_hooked("forward_pre", "backward_pre", "backward"), 1, backward_pre=1)
    assert not pc.quantize_hooks_only(_hooked("forward_pre", "forward_pre")) and pc.quantize_hooks_only(_hooked("forward_pre", "forward_pre"), 2)
    assert not pc.hook_counts(_hooked("forward_pre", "forward_pre"), forward_pre=(0, 1))
    assert pc.hook_counts(both, forward_pre=1, forward=0, backward_pre=1, backward=0) and not pc.hook_counts(both, backward_pre=0)


def _held(n):
    mod = nn.Linear(4, 4)
    mod.activation_pre_process = nn.ModuleDict({str(i): nn.Identity() for i in range(n)})
    return mod, [mod.activation_pre_process[str(i)] for i in range(n)]


def test_holder_lookups():
    h = "activation_pre_process"
    for n in range(4):
        mod, fqs = _held(n)
        assert pc.holder_fqs(mod, h, "0") == ((fqs[0],) if n == 1 else None)
        assert pc.holder_fqs(mod, h, "0", "1") == (tuple(fqs) if n == 2 else None)
        assert pc.holder_fqs(mod, h, "1", "0") == ((fqs[1], fqs[0]) if n == 2 else None)
        assert pc.holder_fqs(mod, h, "0", exact=False) == ((fqs[0],) if n >= 1 else None)
        assert pc.holder_fqs(mod, h, "0", "1", exact=False) == (tuple(fqs[:2]) if n >= 2 else None)
        assert pc.holder_fq(mod, h) is (fqs[0] if n >= 1 else None)
        assert pc.holder_fq(mod, h, "1") is (fqs[1] if n >= 2 else None)
        assert pc.holder_fq(mod, h, exact=True) is (fqs[0] if n == 1 else None)
        assert pc.holder_fqs(mod, "error_pre_process", "0") is None and pc.holder_fq(mod, "error_pre_process") is None
        # the input fake-quantizer of a Linear: exactly {"0"}, and one forward pre-hook (whatever else is hooked) or a prepared Linear
        assert pc.linear_input_fq(mod) is None
        mod.register_forward_pre_hook(lambda m, a: None)
        mod.register_forward_hook(lambda m, a, o: None)
        assert pc.linear_input_fq(mod) is (fqs[0] if n == 1 else None)
        mod.register_forward_pre_hook(lambda m, a: None)
        assert pc.linear_input_fq(mod) is None
        mod.__dict__["_qt_prepared"] = True
        assert pc.linear_input_fq(mod) is (fqs[0] if n == 1 else None)
    assert pc.holder_fqs(None, h, "0") is None and pc.holder_fq(None, h) is None and pc.holder_fqs(nn.Linear(4, 4), h, "0") is None


def _fq(spec, **kw):
    return qt.FusedAmaxObsFakeQuantize(**{**asdict(qt.QuantizationSpec.from_str(spec)), **kw})


def test_plain_per_tensor():
    assert pc.plain_per_tensor(_fq("e4m3")) is True and pc.plain_per_tensor(_fq("int8,qs=per_tensor_symmetric")) is True
    assert pc.plain_per_tensor(_fq("posit8_1")) is True
    assert pc.plain_per_tensor(_fq("int8,qs=per_channel_symmetric,ax=0")) is False
    assert pc.plain_per_tensor(_fq("int8,qs=per_tensor_symmetric,outlier=6.0")) is False
    assert pc.plain_per_tensor(_fq("int8,qs=per_tensor_symmetric", record_histogram=True)) is False
    assert pc.plain_per_tensor(_fq("int8,qs=microscaling,bs=32")) is False
    assert pc.plain_per_tensor(_fq("int8,qs=group_wise_affine,bs=32")) is False
    assert pc.plain_per_tensor(nn.Identity()) is False and pc.plain_per_tensor(None) is False


# ---- what the planners answer when a user hooks a module -------------------------------------------------------------------------------
IDS = torch.randint(3, 97, (2, 16), generator=torch.Generator().manual_seed(0))


def _tiny(name):
    pytest.importorskip("transformers")
    torch.manual_seed(0)
    if name == "bert":
        from transformers import BertConfig, BertForQuestionAnswering
        model = BertForQuestionAnswering(BertConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, vocab_size=100,
                                                    max_position_embeddings=64))
    else:
        from transformers import LlamaConfig, LlamaModel
        model = LlamaModel(LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                                       vocab_size=97, max_position_embeddings=32, attn_implementation="eager"))
    model = model.eval().bfloat16()
    qt.quantize(model, qt.add_qspec_args().parse_args(["--activation", "e4m3", "--weight", "e4m3", "--bf16"]))
    with torch.no_grad():
        model(IDS)                                                           # the first call creates the fake-quantizers
    layer = model.bert.encoder.layer[0] if name == "bert" else model.layers[0]
    norm, attn = (layer.attention.output.LayerNorm, layer.attention.self) if name == "bert" else (layer.input_layernorm, layer.self_attn)
    return norm, attn, norm.__dict__["_qt_consumers"]


def _kind(fq):
    return None if fq is None else "map" if isinstance(fq, tuple) else f"all {len(fq)}" if isinstance(fq, list) else "one"


# Evaluated on the parent commit, case by case (CPU tensors: the attention entry points decline them whatever is hooked).  A forward hook
# on the norm or on a consumer's fake-quantizer costs the codes-only hand-over; the fake-quantizer the norm kernel applies (consumer_fq,
# _norm_consumer_fq) and the rotary kernel's pair (_qk_fqs) do not look at those hooks, and nothing here looks at the softmax.
@pytest.mark.parametrize("hooked, codes_only", [("nothing", True), ("norm", False), ("softmax", True), ("consumer fake-quantizer", False)])
@pytest.mark.parametrize("name, consumers, norm_fq", [("bert", 1, "one"), ("llama", 3, "all 3")])
def test_planner_answers_with_a_user_forward_hook(name, consumers, norm_fq, hooked, codes_only):
    norm, attn, linears = _tiny(name)
    target = {"nothing": None, "norm": norm, "softmax": attn.softmax, "consumer fake-quantizer": linears[0].activation_pre_process["0"]}[hooked]
    if target is not None:
        target.register_forward_hook(lambda m, a, o: None)
    q = torch.zeros(2, 4, 16, 16, dtype=torch.bfloat16)
    with torch.no_grad():
        assert len(linears) == consumers
        assert mf.codes_only_ok(linears, norm) is codes_only
        assert [mf.consumer_fq(lin) is lin.activation_pre_process["0"] for lin in linears] == [True] * consumers
        assert _kind(mf._norm_consumer_fq(norm, allow_all=True, allow_map=name == "llama")) == norm_fq
        assert mf._qk_fqs(attn) == (attn.qk_matmul.activation_pre_process["0"], attn.qk_matmul.activation_pre_process["1"])
        assert attention_route.fused_attention_or_none(attn, q, q, q, None, 0.25, 0.0) is None
        assert attention_route.fused_scores_to_probs_or_none(attn, q, None, 0.25, 0.0, q) is None
