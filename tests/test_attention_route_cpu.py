"""attention_route.AttentionMask.of: which additive masks the attention kernels consume in place, and with which element strides."""
import pytest
import torch

from quantized_training.attention_route import AttentionMask

B, H, Q, C = 2, 4, 8, 16
CPU = torch.device("cpu")


def _mask(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype)


@pytest.mark.parametrize("shape,align,strides", [
    ((2, 1, 8, 16), 8, (128, 0, 16)),
    ((1, 1, 8, 24), 8, (0, 0, 24)),                       # sliced to the key count: the rows keep their pitch
    ((2, 1, 1, 16), 4, (16, 0, 0)),
])
def test_consumable_masks_and_their_strides(shape, align, strides):
    mask = _mask(*shape)
    mk = AttentionMask.of(mask, B, H, Q, C, CPU, align)
    assert mk.strides == strides
    assert mk.owner is mask and mk.view.shape == (*shape[:3], C) and mk.ptr == mask.data_ptr() == mk.view.data_ptr()


@pytest.mark.parametrize("mask,align", [
    (_mask(1, 1, 8, 20), 8),                              # a row pitch of 20 elements is no multiple of 8
    (_mask(2, 1, 8, 16, dtype=torch.float32), 4),
    (_mask(3, 1, 8, 16), 4),                              # batch 3 against B = 2
])
def test_masks_that_cannot_be_consumed_in_place(mask, align):
    assert AttentionMask.of(mask, B, H, Q, C, CPU, align) is None


def test_no_mask_is_a_null_pointer_with_zero_strides():
    mk = AttentionMask.of(None, B, H, Q, C, CPU, 4)
    assert mk is not None and mk.view is None and mk.ptr is None and mk.strides == (0, 0, 0) and mk.owner is None
    assert mk.row_live(B, H, Q, C, None) == (None, 0, 0, 0, None)


@pytest.mark.parametrize("align", [4, 8])
def test_a_mask_that_requires_grad_is_declined_by_the_training_launches_only(align):
    mask = _mask(2, 1, 8, 16).requires_grad_()
    assert AttentionMask.of(mask, B, H, Q, C, CPU, align, no_grad=True) is None
    assert AttentionMask.of(mask, B, H, Q, C, CPU, align).strides == (128, 0, 16)
