"""The producer-to-consumer hand-over protocol (quantized_training/handover.py) on CPU tensors: it needs no device."""
import gc

import torch

from quantized_training import handover
from quantized_training._native import QtFormat

E4M3 = QtFormat(0, 1, 0, 0.0, 0.0)
E5M2 = QtFormat(0, 2, 0, 0.0, 0.0)
CODES = [0x38, 0x40, 0xC0, 0x7E]          # E4M3: 1, 2, -2, 448


def _codes(shape=(4,)):
    n = 1
    for s in shape:
        n *= s
    return handover.fp8_view(torch.tensor((CODES * n)[:n], dtype=torch.uint8).reshape(shape), E4M3)


def test_fp8_view_picks_e5m2_exactly_when_p0_is_2():
    t8 = torch.tensor(CODES, dtype=torch.uint8)
    v = handover.fp8_view(t8, E4M3)
    assert v.dtype == torch.float8_e4m3fn and v.to(torch.bfloat16).tolist() == [1.0, 2.0, -2.0, 448.0]
    assert handover.fp8_view(t8, E5M2).dtype == torch.float8_e5m2
    for p0 in (0, 1, 3, 4):
        assert handover.fp8_view(t8, QtFormat(0, p0, 0, 0.0, 0.0)).dtype == torch.float8_e4m3fn

    class Holder:                          # a fake-quantizer carries its format
        _qt_format = E5M2
    assert handover.fp8_view(t8, Holder()).dtype == torch.float8_e5m2
    assert handover.fp8_view(t8, E4M3).data_ptr() == t8.data_ptr()


def test_stamp_then_inplace_write_makes_everything_stale():
    t, src = torch.zeros(4, dtype=torch.bfloat16), torch.ones(4, dtype=torch.bfloat16)
    fq, other, c = object(), object(), _codes()
    assert not handover.valid(t) and handover.codes(t) is None and handover.done_by(t) is None and handover.origin(t) is None
    assert handover.stamp(t, fq, c, also=[(other, c)], origin=handover.tensor_key(src)) is t
    assert handover.valid(t) and handover.codes(t) is c and handover.done_by(t) is fq
    assert handover.also_done(t) == [(other, c)] and handover.origin(t) == (src.data_ptr(), src._version, (4,))
    assert t._qt_fp8 is c and t._qt_fq_done_by is fq and t._qt_ver == t._version and not handover.is_lazy(t)
    t.add_(1)
    assert not handover.valid(t)
    assert handover.codes(t) is None and handover.done_by(t) is None and handover.origin(t) is None and handover.also_done(t) is None
    assert handover.codes(t, unchecked=True) is c and handover.done_by(t, unchecked=True) is fq       # the explicit door stays open


def test_tensor_key_follows_address_version_and_shape():
    t = torch.zeros(2, 3)
    k = handover.tensor_key(t)
    assert k == (t.data_ptr(), t._version, (2, 3)) and handover.tensor_key(t.view(2, 3)) == k
    assert handover.tensor_key(t.view(3, 2)) != k and handover.tensor_key(t[1:]) != k
    t.mul_(2)
    assert handover.tensor_key(t) != k


def test_mark_lazy_poisons_and_materialize_decodes(monkeypatch):
    monkeypatch.setenv("QT_LAZY_POISON", "1")
    t = torch.zeros(4, dtype=torch.bfloat16)
    fq = object()
    handover.stamp(t, fq, _codes(), lazy=True)
    assert handover.is_lazy(t) and t._qt_lazy is True and torch.isnan(t).all()
    assert handover.valid(t) and handover.done_by(t) is fq          # the fill is not a modification of the result
    handover.materialize(t)
    assert t.tolist() == [1.0, 2.0, -2.0, 448.0]
    assert not handover.is_lazy(t) and handover.valid(t) and handover.done_by(t) is fq
    before = t._version
    handover.materialize(t)                                         # nothing left to do
    assert t._version == before
    # marking a stamped tensor afterwards keeps it valid too; without the variable nothing is written
    u = handover.stamp(torch.zeros(4, dtype=torch.bfloat16), fq, _codes())
    handover.mark_lazy(u)
    assert torch.isnan(u).all() and handover.valid(u) and handover.is_lazy(u)
    monkeypatch.setenv("QT_LAZY_POISON", "0")
    w = handover.stamp(torch.zeros(4, dtype=torch.bfloat16), fq, _codes(), lazy=True)
    assert handover.is_lazy(w) and w._version == 0 and w.tolist() == [0.0] * 4


def test_view_of_a_lazy_tensor_is_materialized_through_the_registry(monkeypatch):
    monkeypatch.setenv("QT_LAZY_POISON", "1")
    t = handover.stamp(torch.zeros(2, 4, dtype=torch.bfloat16), object(), _codes((2, 4)), lazy=True)
    assert t.data_ptr() in handover._LAZY
    # same address, another dtype or another extent: not this tensor's values
    as_int = t.view(torch.int16)
    part = t[0]
    handover.materialize(as_int)
    handover.materialize(part)
    assert handover.is_lazy(t) and torch.isnan(t).all()
    for view in (t.view(8), t.reshape(4, 2)):
        assert not hasattr(view, "_qt_lazy")
    v = t.view(8)
    handover.stamp(v, origin=handover.tensor_key(t))
    handover.materialize(v)
    assert v.tolist() == [1.0, 2.0, -2.0, 448.0] * 2 and not handover.is_lazy(t) and handover.valid(t)
    assert handover.valid(v)                                        # a stamped view stays stamped through the decode
    t2 = handover.stamp(torch.zeros(2, 4, dtype=torch.bfloat16), object(), _codes((2, 4)), lazy=True)
    r = t2.reshape(4, 2)
    handover.materialize(r)
    assert r.reshape(-1).tolist() == [1.0, 2.0, -2.0, 448.0] * 2 and not handover.valid(r)
    # the entry dies with the tensor
    ptr = t2.data_ptr()
    assert ptr in handover._LAZY
    del t2, r
    gc.collect()
    assert ptr not in handover._LAZY
    # flag alone (register=False): no poison, no registry entry
    b = handover.stamp(torch.zeros(4, dtype=torch.bfloat16), object(), _codes(), lazy=True, register=False)
    assert handover.is_lazy(b) and handover.valid(b) and b.tolist() == [0.0] * 4 and b.data_ptr() not in handover._LAZY


def test_carry_is_a_view_with_origin_and_inherits_lazy():
    X, src = torch.arange(8, dtype=torch.bfloat16), torch.zeros(2, 4, dtype=torch.bfloat16)
    c = _codes((2, 4))
    out = handover.carry(X, c, src)
    assert out is not X and out.data_ptr() == X.data_ptr() and out.shape == src.shape
    assert out.untyped_storage().data_ptr() == X.untyped_storage().data_ptr()
    assert handover.valid(out) and handover.codes(out) is c and handover.origin(out) == handover.tensor_key(src)
    assert out._qt_origin == (src.data_ptr(), src._version, (2, 4))
    assert handover.done_by(out) is None and not handover.is_lazy(out) and not hasattr(X, "_qt_fp8")
    handover.stamp(X, object(), c.view(8), lazy=True)
    lazy = handover.carry(X, c.view(8), X)
    assert lazy.shape == X.shape and handover.is_lazy(lazy) and handover.valid(lazy)
    handover.materialize(lazy)                                      # decodes into the shared storage
    assert X.tolist() == [1.0, 2.0, -2.0, 448.0] * 2


def test_transposed_hands_k_to_its_transpose_unless_stale():
    fq = object()
    key = torch.zeros(1, 2, 3, 4, dtype=torch.bfloat16)
    c = _codes((1, 2, 3, 4))
    handover.stamp(key, fq, c)
    key_t = key.transpose(2, 3)
    assert handover.transposed(key, key_t) is key_t
    assert handover.valid(key_t) and handover.done_by(key_t) is fq and handover.codes_of_transpose(key_t) is c
    assert handover.codes(key_t) is None and key_t._qt_fp8_of_transpose is c
    # done-by without codes (table formats): the transposed view is done as well, with no codes to carry
    plain = handover.stamp(torch.zeros(1, 2, 3, 4, dtype=torch.bfloat16), fq)
    plain_t = handover.transposed(plain, plain.transpose(2, 3))
    assert handover.done_by(plain_t) is fq and handover.codes_of_transpose(plain_t) is None
    # codes without a done-by (a fake-quantizer's own pass): nothing to say about K^T
    own = handover.stamp(torch.zeros(1, 2, 3, 4, dtype=torch.bfloat16), codes=c)
    own_t = handover.transposed(own, own.transpose(2, 3))
    assert not handover.valid(own_t) and not hasattr(own_t, "_qt_fp8_of_transpose")
    key.add_(1)
    stale_t = handover.transposed(key, key.transpose(2, 3))
    assert not handover.valid(stale_t) and handover.done_by(stale_t, unchecked=True) is None
    assert not hasattr(stale_t, "_qt_fp8_of_transpose")
    assert not handover.valid(key_t)                                # the earlier view shares the version counter
