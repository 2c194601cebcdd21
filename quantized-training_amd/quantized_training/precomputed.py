"""Results computed ahead of the call that asks for them: some launch evaluated a call before it was issued and leaves a note, so that the
call returns the result instead of computing it.  handover.py owns the records that travel ON a result tensor; this module owns the
records left for a FUTURE call, and is the only code that reads or writes them.  It imports handover.tensor_key and nothing else from the
package.

  PRE           fq(W) of a weight fake-quantizer's next call      fake_quantize.BatchedWeightFakeQuant, model_fusions.rope_map
  EXPECTED      fq(tensor) a producing kernel wrote               FusedAmaxObsFakeQuantize.expect_prequantized
  CHAIN_RESULT  a chain member's result                           train_fusions.run_chain, _hand_over, _served_call
  WEIGHT_CODES  the FP8 weight codes of a Linear / SiblingGroup   fused.BatchedWeightCodes
  COLSUM        column sums of a grad_output (the bias gradient)  train_fusions.put_colsum / take_colsum
  LINEAR_GRADS  (grad_input, grad_weight) of a q / k / v Linear   train_fusions.group_qkv_backward / take_linear_grads
  VALUE_CODES_T (fq_v, V^T as FP8 codes) for qt_attention_fp8     `_qt_vt8`: model_fusions.rope_fq, pt2e_fusion / attention_route
  VALUE_T_ROWS  (fq_v, fq_v(V)^T) for qt_attention_rows_bf16      `_qt_vt_rows`: model_fusions.rope_map / attention_route
  the amax histories whose next scale update is already done      mark_preupdated / take_preupdate / forget_preupdated

Every record is ONE SHOT (looking it up removes it, hit or not) and names the tensor(s) the future call must receive by address and
version counter; it also HOLDS them, so that no address can be handed to another tensor while the record exists.  A record that does
not match is a miss, never an error: the call computes as usual.

Stays where it is (its lifetime is not that of a one-shot record keyed by a tensor):
  train_fusions._PENDING / _HOLDS          follow the autograd graph's token, not a capacity
  `_qt_deferred`                           an arm flag, not a tensor key
  modules/qat/linear.py _FWD_PENDING, `_qt_train_xw`      launches not yet issued / weak references to a node's operands
  fused.SiblingGroup.stash                 shared by several takers"""
from collections import namedtuple

from .handover import tensor_key

Record = namedtuple("Record", "key tensors payload")
MISS = object()           # Slot.take: there was a record, for other contents than the call received


def _numel_key(t):
    return (t.data_ptr(), t._version, t.numel())


def _versions_key(ts):
    return tuple((t.data_ptr(), t._version) for t in ts)


def _strided_key(t):
    return (*tensor_key(t), t.stride())


# rule -> (key of the tensor(s), the layout the call's tensor must have beside an equal key)
_RULES = {"shape": (tensor_key, lambda X, kept: X.is_contiguous() or X.stride() == kept.stride()),
          "numel": (_numel_key, lambda X, kept: X.is_contiguous()),
          "versions": (_versions_key, lambda Xs, kept: True),           # several tensors: one (address, version) per member
          "strided": (_strided_key, lambda X, kept: True)}              # a view a kernel reads in place: the same strides too


class Slot:
    """A named one-shot record in the `__dict__` of the object whose future call it serves."""

    def __init__(self, name, rule):
        self.name = name
        self._key, self._layout = _RULES[rule]

    def leave(self, owner, tensors, payload):
        owner.__dict__[self.name] = Record(self._key(tensors), tensors, payload)

    def take(self, owner, X):
        """None: nothing was left; MISS: something was, for other contents than X; else the payload.  The record is gone in every case."""
        rec = owner.__dict__.pop(self.name, None)
        if rec is None:
            return None
        return rec.payload if self._key(X) == rec.key and self._layout(X, rec.tensors) else MISS

    def drop(self, owner):
        owner.__dict__.pop(self.name, None)

    def peek(self, owner):
        return owner.__dict__.get(self.name)


PRE = Slot("_qt_pre", "shape")
EXPECTED = Slot("_qt_expected", "numel")
CHAIN_RESULT = Slot("_qt_chain_result", "shape")
WEIGHT_CODES = Slot("_qt_w8_pre", "versions")
VALUE_CODES_T = Slot("_qt_vt8", "strided")            # payload (fq_v, vt): the taker accepts it only for its own fq_v
VALUE_T_ROWS = Slot("_qt_vt_rows", "strided")


class Table:
    """One-shot records keyed by the tensor a backward node will receive.  At capacity the OLDEST entry leaves, never all of them: its
    taker computes for itself.  `ident`: a second identity the taker must present; another one consumes the entry and answers nothing."""

    def __init__(self, capacity):
        self.capacity = capacity
        self._entries = {}

    def put(self, t, payload, ident=None):
        while len(self._entries) >= self.capacity:
            del self._entries[next(iter(self._entries))]
        self._entries[tensor_key(t)] = (t, ident, payload)

    def take(self, t, ident=None):
        hit = self._entries.pop(tensor_key(t), None)
        return hit[2] if hit is not None and hit[1] == ident else None

    def __len__(self):
        return len(self._entries)

    def clear(self):
        self._entries.clear()


COLSUM = Table(64)
LINEAR_GRADS = Table(16)


_PREUPDATED = set()       # data_ptr of every amax history whose NEXT call's delayed-scaling update has already been done


def mark_preupdated(hist):
    _PREUPDATED.add(hist.data_ptr())


def take_preupdate(hist) -> bool:
    p = hist.data_ptr()
    if p in _PREUPDATED:
        _PREUPDATED.discard(p)
        return True
    return False


def forget_preupdated(hist):
    _PREUPDATED.discard(hist.data_ptr())
