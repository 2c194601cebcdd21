"""The records left for a future call (quantized_training/precomputed.py) and the allocator of tensors handed out before they are
written (handover.unwritten), on CPU tensors: they need no device."""
import pytest
import torch

from quantized_training import handover, precomputed
from quantized_training.fake_quantize import STATS, FusedAmaxObsFakeQuantize
from quantized_training.precomputed import MISS, Slot, Table


class Owner:
    pass


SHAPE = Slot("_test_shape", "shape")
NUMEL = Slot("_test_numel", "numel")
SEVERAL = Slot("_test_several", "versions")
STRIDED = Slot("_test_strided", "strided")


# ---- Slot ------------------------------------------------------------------------------------------------------------------------
def test_shape_slot_hits_the_very_tensor_once():
    o, t = Owner(), torch.zeros(4, 6)
    assert SHAPE.peek(o) is None and SHAPE.take(o, t) is None                # nothing left: "no record", not a miss
    SHAPE.leave(o, t, "result")
    rec = SHAPE.peek(o)
    assert rec.key == handover.tensor_key(t) and rec.tensors is t and rec.payload == "result"
    assert SHAPE.peek(o) is rec                                              # looking does not take
    assert SHAPE.take(o, t) == "result"
    assert SHAPE.peek(o) is None and SHAPE.name not in o.__dict__
    assert SHAPE.take(o, t) is None                                          # one shot
    SHAPE.leave(o, t, "again")
    assert SHAPE.take(o, t.view(4, 6)) == "again"                            # a view with the same contents, extent and layout is that tensor


def test_shape_slot_misses_and_clears_on_other_contents():
    o, t = Owner(), torch.zeros(4, 6)
    for other in (lambda: torch.zeros(4, 6), lambda: t.view(6, 4), lambda: t.view(24), lambda: t[1:]):
        SHAPE.leave(o, t, "result")
        assert SHAPE.take(o, other()) is MISS
        assert SHAPE.peek(o) is None and SHAPE.take(o, t) is None            # a miss clears the record too
    SHAPE.leave(o, t, "result")
    t.add_(1)                                                                # another version of the same tensor is other contents
    assert SHAPE.take(o, t) is MISS and SHAPE.peek(o) is None
    SHAPE.leave(o, t, "result")
    SHAPE.drop(o)
    assert SHAPE.peek(o) is None and SHAPE.take(o, t) is None
    SHAPE.drop(o)                                                            # nothing to drop: fine


def test_shape_slot_takes_a_strided_tensor_only_with_the_kept_strides():
    o = Owner()
    base = torch.zeros(6, 4)
    kept = base.t()                                                          # [4, 6], strides (1, 4)
    assert not kept.is_contiguous()
    SHAPE.leave(o, kept, "result")
    assert SHAPE.take(o, base.t()) == "result"                               # another view object, strided like the kept tensor
    SHAPE.leave(o, kept, "result")
    other = base.view(4, 6)                                                  # same address, version and shape; contiguous
    assert handover.tensor_key(other) == handover.tensor_key(kept)
    assert SHAPE.take(o, other) == "result"                                  # (the rule as it always was: X contiguous OR strided like the kept one)
    wide = torch.zeros(4, 12)
    SHAPE.leave(o, wide[:, :6], "result")                                    # strides (12, 1)
    sparse = wide[:, ::2]                                                    # same address, version, shape; strides (12, 2)
    assert handover.tensor_key(sparse) == handover.tensor_key(wide[:, :6]) and not sparse.is_contiguous()
    assert SHAPE.take(o, sparse) is MISS


def test_numel_slot_takes_a_contiguous_view_of_another_shape():
    o, t = Owner(), torch.zeros(2, 3, 4)
    NUMEL.leave(o, t, "result")
    assert NUMEL.peek(o).key == (t.data_ptr(), t._version, 24)
    assert NUMEL.take(o, t.view(6, 4)) == "result" and NUMEL.take(o, t.view(6, 4)) is None
    NUMEL.leave(o, t, "result")
    assert NUMEL.take(o, t.permute(2, 0, 1)) is MISS                         # same address, version, extent: not contiguous
    NUMEL.leave(o, t, "result")
    assert NUMEL.take(o, t[0]) is MISS                                       # another extent
    NUMEL.leave(o, t, "result")
    t.mul_(2)
    assert NUMEL.take(o, t) is MISS
    base = torch.zeros(6, 4)
    NUMEL.leave(o, base.t(), "result")                                       # the shape rule would take this one; this rule wants it contiguous
    assert NUMEL.take(o, base.t()) is MISS


def test_strided_slot_takes_the_very_view_with_the_very_strides():
    """The rule of the value pass a rotary launch writes ahead of the attention core (VALUE_CODES_T, VALUE_T_ROWS): the kernels read the
    [B, H, S, D] view of a projection's output in place, so another stride over the same storage is another tensor."""
    assert precomputed.VALUE_CODES_T.name == "_qt_vt8" and precomputed.VALUE_T_ROWS.name == "_qt_vt_rows"
    o, fq = Owner(), object()
    buf = torch.zeros(2, 8, 3 * 4 * 16)                                      # [B, S, 3 * H * D]: q | k | v
    value = buf[:, :, 128:].view(2, 8, 4, 16).transpose(1, 2)                # [B, H, S, D]
    for slot in (STRIDED, precomputed.VALUE_CODES_T, precomputed.VALUE_T_ROWS):
        assert slot.take(o, value) is None
        slot.leave(o, value, (fq, "vt"))
        rec = slot.peek(o)
        assert rec.key == (*handover.tensor_key(value), value.stride()) and rec.tensors is value
        again = buf[:, :, 128:].view(2, 8, 4, 16).transpose(1, 2)            # another view object of the same contents
        assert slot.take(o, again) == (fq, "vt")
        assert slot.peek(o) is None and slot.take(o, value) is None          # gone after the take
        slot.leave(o, value, (fq, "vt"))
        narrow = torch.as_strided(buf, value.shape, (value.stride(0), 8, value.stride(2), 1), value.storage_offset())
        assert handover.tensor_key(narrow) == handover.tensor_key(value) and narrow.stride() != value.stride()
        assert slot.take(o, narrow) is MISS                                  # the same storage seen through another stride
        assert slot.peek(o) is None and slot.take(o, value) is None          # gone after a miss too
        slot.leave(o, value, (fq, "vt"))
        assert slot.take(o, value.contiguous()) is MISS                      # a copy: another address
        slot.leave(o, value, (fq, "vt"))
        buf.add_(1)                                                          # a bumped version: other contents
        assert slot.take(o, value) is MISS and slot.peek(o) is None
        slot.leave(o, value, (fq, "vt"))
        slot.drop(o)
        assert slot.peek(o) is None and slot.take(o, value) is None


def test_strided_slot_holds_its_tensor_while_it_exists():
    o = Owner()
    t = torch.randn(2, 4, 8, 16)
    STRIDED.leave(o, t, ("fq", "vt"))
    ptr = t.data_ptr()
    del t
    others = [torch.randn(2, 4, 8, 16) for _ in range(32)]
    assert all(x.data_ptr() != ptr for x in others)                          # no later tensor is placed at the recorded address ...
    assert STRIDED.peek(o).tensors.data_ptr() == ptr
    assert STRIDED.take(o, others[0]) is MISS                                # ... so none can match the record


def test_slot_over_several_tensors_sits_on_its_owner():
    o = Owner()
    ws = [torch.zeros(3, 8), torch.zeros(5, 8), torch.zeros(3, 8)]
    SEVERAL.leave(o, ws, "codes")
    assert SEVERAL.peek(o).key == tuple((w.data_ptr(), w._version) for w in ws)
    assert SEVERAL.take(o, tuple(ws)) == "codes" and SEVERAL.take(o, ws) is None
    SEVERAL.leave(o, ws, "codes")
    ws[1].add_(1)                                                            # one member's version bump
    assert SEVERAL.take(o, ws) is MISS and SEVERAL.peek(o) is None
    SEVERAL.leave(o, ws, "codes")
    assert SEVERAL.take(o, ws[:2]) is MISS                                   # other members
    SEVERAL.leave(o, ws, "codes")
    assert SEVERAL.take(o, [ws[0], ws[2], ws[1]]) is MISS
    # the record lives on the owner: an owner that goes takes it along, and whatever object comes next -- at the same address or not --
    # starts without one (a table keyed by id(owner) could not promise that)
    SEVERAL.leave(o, ws, "codes")
    del o
    for _ in range(32):
        fresh = Owner()
        assert SEVERAL.peek(fresh) is None and SEVERAL.take(fresh, ws) is None


def test_a_record_keeps_its_tensors_storage():
    o = Owner()
    t = torch.randn(4, 8)
    SHAPE.leave(o, t, "result")
    ptr = t.data_ptr()
    del t
    others = [torch.randn(4, 8) for _ in range(32)]
    assert all(x.data_ptr() != ptr for x in others)                          # the record holds the tensor: its address is not handed out again
    for x in others:
        assert SHAPE.peek(o).key[0] == ptr and handover.tensor_key(x) != SHAPE.peek(o).key
    assert SHAPE.take(o, others[0]) is MISS
    several = [torch.randn(4, 8), torch.randn(4, 8)]
    ptrs = [x.data_ptr() for x in several]
    SEVERAL.leave(o, several, "codes")
    del several
    assert all(x.data_ptr() not in ptrs for x in [torch.randn(4, 8) for _ in range(32)])


# ---- Table -----------------------------------------------------------------------------------------------------------------------
def test_table_never_matches_another_tensor_and_evicts_the_oldest():
    table = Table(64)
    g = torch.randn(4, 8)
    table.put(g, "sums of g")
    ptr = g.data_ptr()
    del g
    others = [torch.randn(4, 8) for _ in range(32)]
    assert all(t.data_ptr() != ptr for t in others)                          # the entry keeps the storage alive
    assert all(table.take(t) is None for t in others)
    keep = []
    for i in range(70):
        t = torch.randn(2, 8)
        keep.append(t)
        table.put(t, i)
    assert len(table) == 64
    assert table.take(keep[-1]) == 69 and table.take(keep[-1]) is None       # one shot
    assert table.take(keep[10]) == 10 and table.take(keep[0]) is None        # the oldest went, the others stayed
    assert all(table.take(keep[i]) is None for i in range(6))                # 1 + 70 puts into 64 places: the first seven went ...
    assert table.take(keep[6]) == 6                                          # ... and no more than those
    t = keep[20]
    t.add_(1.0)                                                              # another version of the same tensor is another gradient
    assert table.take(t) is None
    table.clear()
    assert len(table) == 0 and table.take(keep[30]) is None


def test_table_with_ident_consumes_on_a_mismatch():
    table = Table(16)
    keep = []
    for i in range(20):
        t = torch.randn(2, 8)
        keep.append(t)
        table.put(t, ("gx", i), ident=("x and w of", i))
    assert len(table) == 16
    assert all(table.take(keep[i], ("x and w of", i)) is None for i in range(4))          # the oldest four went
    assert len(table) == 16
    assert table.take(keep[19], ("x and w of", 19)) == ("gx", 19) and table.take(keep[19], ("x and w of", 19)) is None
    assert table.take(keep[10], ("x and w of", 11)) is None                  # another identity: nothing ...
    assert len(table) == 14 and table.take(keep[10], ("x and w of", 10)) is None          # ... and the entry is consumed
    assert table.take(keep[12]) is None and len(table) == 13                 # no identity presented where one was left: the same
    keep[15].add_(1.0)
    assert table.take(keep[15], ("x and w of", 15)) is None and len(table) == 13          # another version was never in the table
    table.clear()
    assert len(table) == 0


def test_the_package_tables_have_their_capacities():
    assert precomputed.COLSUM.capacity == 64 and precomputed.LINEAR_GRADS.capacity == 16


# ---- the "scale already updated" set ----------------------------------------------------------------------------------------------------
def test_preupdate_is_marked_once_taken_once_and_forgotten():
    h, other = torch.zeros(4), torch.zeros(4)
    assert not precomputed.take_preupdate(h)
    precomputed.mark_preupdated(h)
    precomputed.mark_preupdated(h)                                           # marking twice is one mark
    assert not precomputed.take_preupdate(other)
    assert precomputed.take_preupdate(h) and not precomputed.take_preupdate(h)
    precomputed.mark_preupdated(h)
    precomputed.forget_preupdated(h)
    precomputed.forget_preupdated(h)                                         # nothing to forget: fine
    assert not precomputed.take_preupdate(h)


# ---- handover.unwritten ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", ["0", "1"])
def test_unwritten_is_nan_exactly_when_poisoned(poison, monkeypatch):
    monkeypatch.setenv("QT_LAZY_POISON", poison)
    like = torch.zeros(3, 5, dtype=torch.float64)
    for t, shape, dtype in ((handover.unwritten((2, 7), torch.bfloat16, torch.device("cpu")), (2, 7), torch.bfloat16),
                            (handover.unwritten(like=like), (3, 5), torch.float64)):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == "cpu" and t.is_contiguous()
        assert t.data_ptr() != like.data_ptr()
        if poison == "1":
            assert torch.isnan(t).all()
    assert like.tolist() == [[0.0] * 5] * 3                                  # `like` is a pattern, not a target
    mine = torch.zeros(4)
    assert handover.unwritten(out=mine) is mine
    assert torch.isnan(mine).all() if poison == "1" else mine.tolist() == [0.0] * 4


# ---- FusedAmaxObsFakeQuantize.forward with a record left -----------------------------------------------------------------------------------
def _weight():
    return (torch.randn(8, 16, generator=torch.Generator().manual_seed(3)) * 4).bfloat16()


def test_forward_returns_what_was_left_for_this_weight():
    fq = FusedAmaxObsFakeQuantize(dtype="e4m3")
    W = _weight()
    want = fq(W).clone()
    out = torch.full_like(W, 7.0)                                            # (a marker: the call must hand THIS tensor out, not compute)
    precomputed.PRE.leave(fq, W, out)
    STATS.reset()
    got = fq(W)
    assert got.untyped_storage().data_ptr() == out.untyped_storage().data_ptr() and got.shape == W.shape and (got == 7.0).all()
    assert STATS.elements == W.numel()
    assert precomputed.PRE.peek(fq) is None
    STATS.reset()
    assert torch.equal(fq(W), want) and STATS.elements == W.numel()          # the record was for one call


def test_forward_recomputes_after_the_weight_changed_in_place():
    fq = FusedAmaxObsFakeQuantize(dtype="e4m3")
    W = _weight()
    out = torch.full_like(W, 7.0)
    precomputed.PRE.leave(fq, W, out)
    W.mul_(2)
    want = FusedAmaxObsFakeQuantize(dtype="e4m3")(W)
    STATS.reset()
    got = fq(W)
    assert got.untyped_storage().data_ptr() != out.untyped_storage().data_ptr() and torch.equal(got, want)
    assert STATS.elements == W.numel()
    assert precomputed.PRE.peek(fq) is None                                  # a miss clears it as well


@pytest.mark.parametrize("with_replacement", [False, True])
def test_forward_returns_what_a_producer_announced(with_replacement):
    fq = FusedAmaxObsFakeQuantize(dtype="e4m3")
    y = _weight().reshape(2, 4, 16)
    x8 = torch.arange(y.numel(), dtype=torch.uint8).reshape(y.shape)
    replacement = torch.full_like(y, 5.0) if with_replacement else None
    fq.expect_prequantized(y, x8, replacement=replacement)
    assert precomputed.EXPECTED.peek(fq).tensors is y                        # held until the call
    view = y.reshape(8, 16)                                                  # the hook receives a reshaped view (Python attributes are gone)
    STATS.reset()
    got = fq(view)
    assert STATS.elements == y.numel() and precomputed.EXPECTED.peek(fq) is None
    assert handover.valid(got) and handover.codes(got).data_ptr() == x8.data_ptr()
    if with_replacement:
        assert got.untyped_storage().data_ptr() == replacement.untyped_storage().data_ptr() and got.shape == view.shape
        assert handover.origin(got) == handover.tensor_key(view) and tuple(handover.codes(got).shape) == tuple(view.shape)
    else:
        assert got is view
    # a changed tensor: the call computes, and the record is gone all the same
    fq2 = FusedAmaxObsFakeQuantize(dtype="e4m3")
    fq2.expect_prequantized(y, x8, replacement=replacement)
    y.mul_(2)
    want = FusedAmaxObsFakeQuantize(dtype="e4m3")(view)
    STATS.reset()
    got = fq2(view)
    assert got is not view and torch.equal(got, want) and STATS.elements == y.numel()
    assert got.untyped_storage().data_ptr() not in (y.untyped_storage().data_ptr(), x8.untyped_storage().data_ptr())
    assert replacement is None or got.untyped_storage().data_ptr() != replacement.untyped_storage().data_ptr()
    assert precomputed.EXPECTED.peek(fq2) is None
