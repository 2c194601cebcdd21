"""The block-scaled operand hand-over (quantized_training/mx_operand.py) on CPU tensors: it needs no device."""
import pytest
import torch

from quantized_training import mx_operand as mo
from quantized_training.fake_quantize import _table_for, get_quantization_map

LAYOUTS = (mo.ROWS, mo.SECOND, mo.NHWC)


def _tagged(shape=(2, 4, 8), fid=0, bs=32):
    """Values [.., rows, k] with format, scale flag and the as-stored operand, as the last-axis quantize_mx kernel leaves them."""
    q, s = torch.zeros(shape, dtype=torch.bfloat16), torch.ones(shape[:-1] + (1,), dtype=torch.bfloat16)
    rows = q.numel() // shape[-1]
    codes, e8 = torch.zeros(rows, mo.row_bytes(shape[-1], fid), dtype=torch.uint8), torch.zeros(rows, 1, dtype=torch.uint8)
    mo.quantized(q, s, "fp8_e4m3", mo.ROWS, fid, bs, codes, e8)
    return q, s, codes, e8


# ---- kernel facts ------------------------------------------------------------------------------------------------------------------
ROW_BYTES = {  # format -> bytes of a row of k = 32, 64, 96, 128 elements
    "fp8_e4m3": (32, 64, 96, 128), "fp8_e5m2": (32, 64, 96, 128), "fp6_e2m3": (24, 48, 72, 96), "fp6_e3m2": (24, 48, 72, 96),
    "fp4_e2m1": (16, 32, 48, 64),
}


def test_row_helpers_against_a_literal_table():
    assert mo.FMT_ID == {"fp8_e4m3": 0, "fp8_e5m2": 1, "fp6_e2m3": 2, "fp6_e3m2": 3, "fp4_e2m1": 4}
    for name, want in ROW_BYTES.items():
        fid = mo.FMT_ID[name]
        assert tuple(mo.row_bytes(k, fid) for k in (32, 64, 96, 128)) == want
        whole = tuple(mo.row_is_whole_chunks(k, fid) for k in (32, 64, 96, 128))
        assert whole == ((False, True, False, True) if name.startswith("fp6") else (True,) * 4)
    assert len(mo.PAIRS) == 10 and set(mo.NARROW_FIRST) == set(mo.FMT_ID)


def test_mx_gemm_re_exports_the_facts():
    from quantized_training import mx_gemm
    assert mx_gemm.FMT_ID is mo.FMT_ID and mx_gemm._PAIRS is mo.PAIRS and mx_gemm._BITS is mo.BITS


# ---- writers and readers -----------------------------------------------------------------------------------------------------------
def test_each_writer_round_trips():
    q, s = torch.zeros(4, 64, dtype=torch.bfloat16), torch.ones(4, 2, dtype=torch.bfloat16)
    assert mo.format_of(q) is None and not mo.is_pow2(s) and all(mo.operand_record(q, lay) is None for lay in LAYOUTS)
    assert mo.set_format(q, "fp8_e4m3") is q and mo.format_of(q) == "fp8_e4m3"
    assert mo.set_pow2(s) is s and mo.is_pow2(s) is True
    codes, e8 = torch.zeros(4, 64, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.uint8)
    for layout, raw in zip(LAYOUTS, ("_qt_mx_packed_act", "_qt_mx_packed_b", "_qt_mx_packed_nhwc")):
        mo.drop_operand(q)
        assert mo.set_operand(q, layout, 0, 32, codes, e8) is q
        rec = mo.operand_record(q, layout)
        assert rec[:2] == (0, 32) and rec[2] is codes and rec[3] is e8 and getattr(q, raw) is rec
        got = mo.operand(q, layout, 0, 32, 4, 64)
        assert got[0] is codes and got[1] is e8
        assert all(mo.operand_record(q, other) is None for other in LAYOUTS if other != layout)     # it answers per layout
    assert mo.format_of(q) == "fp8_e4m3"                            # the operand writer leaves the format alone
    assert q._qt_mx_fmt == "fp8_e4m3" and q._qt_mx_ver == q._version and s._qt_pow2 is True and s._qt_mx_ver == s._version
    mo.set_format(q, "int8")                                        # the writer stores the name it is given; consumers test `in FMT_ID`
    assert mo.format_of(q) == "int8" and mo.format_of(q) not in mo.FMT_ID


def test_operand_reader_checks_format_block_rows_and_k():
    q, s, codes, e8 = _tagged((4, 64))
    assert mo.operand(q, mo.ROWS, 0, 32, 4, 64) is not None
    assert mo.operand(q, mo.ROWS, 1, 32, 4, 64) is None             # another format id
    assert mo.operand(q, mo.ROWS, 0, 64, 4, 64) is None             # another block size
    assert mo.operand(q, mo.ROWS, 0, 32, 8, 64) is None             # another row count
    assert mo.operand(q, mo.ROWS, 0, 32, 4, 128) is None            # another k
    assert mo.operand(q, mo.SECOND, 0, 32, 4, 64) is None and mo.operand(q, mo.NHWC, 0, 32, 4, 64) is None


def test_inplace_write_makes_the_whole_record_stale():
    for layout in LAYOUTS:
        q, s, codes, e8 = _tagged((4, 64))
        mo.set_operand(q, layout, 0, 32, codes, e8)
        q.add_(1)
        assert mo.format_of(q) is None and all(mo.operand_record(q, lay) is None for lay in LAYOUTS)
        assert mo.operand(q, layout, 0, 32, 4, 64) is None
        assert mo.is_pow2(s)                                        # the scale is another tensor
        s.mul_(2)
        assert not mo.is_pow2(s)
    # a later writer does not revive what the stale stamp vouched for
    mo.set_format(q, "fp8_e5m2")
    assert mo.format_of(q) == "fp8_e5m2" and all(mo.operand_record(q, lay) is None for lay in LAYOUTS)


def test_drop_operand_keeps_format_and_forget_drops_all():
    q, s, _, _ = _tagged((4, 64))
    assert mo.drop_operand(q) is q
    assert mo.operand_record(q, mo.ROWS) is None and mo.format_of(q) == "fp8_e4m3" and mo.is_pow2(s)
    mo.forget(q), mo.forget(s)
    assert mo.format_of(q) is None and not mo.is_pow2(s) and not mo.valid(q)
    mo.drop_operand(torch.zeros(2))                                 # nothing to drop: no error


# ---- the carry ---------------------------------------------------------------------------------------------------------------------
def test_carry_to_a_transposed_view():
    q, s, codes, e8 = _tagged((2, 4, 8))
    q_t, s_t = q.transpose(-1, -2), s.transpose(-1, -2)
    assert mo.carry(q, s, q_t, s_t) == mo.SECOND
    assert mo.format_of(q_t) == "fp8_e4m3" and mo.is_pow2(s_t)
    rec = mo.operand_record(q_t, mo.SECOND)
    assert rec[:2] == (0, 32) and rec[2] is codes and rec[3] is e8
    assert mo.operand_record(q_t, mo.ROWS) is None and mo.operand_record(q_t, mo.NHWC) is None
    q_t.add_(1)                                                     # a write through the view stales the base ...
    assert mo.format_of(q) is None and mo.operand_record(q, mo.ROWS) is None and mo.format_of(q_t) is None
    q2, s2, _, _ = _tagged((2, 4, 8))
    q2_t, s2_t = q2.transpose(-1, -2), s2.transpose(-1, -2)
    mo.carry(q2, s2, q2_t, s2_t)
    q2.add_(1), s2.mul_(2)                                          # ... and the reverse
    assert mo.format_of(q2_t) is None and mo.operand_record(q2_t, mo.SECOND) is None and not mo.is_pow2(s2_t)


def test_carry_to_a_permuted_view():
    q, s, codes, e8 = _tagged((2, 3, 4, 8))                         # stored [N, H, W, C]
    q_p, s_p = q.permute(0, 3, 1, 2), s.permute(0, 3, 1, 2)
    assert mo.carry(q, s, q_p, s_p) == mo.NHWC
    assert mo.operand_record(q_p, mo.NHWC)[2] is codes and mo.format_of(q_p) == "fp8_e4m3" and mo.is_pow2(s_p)
    assert mo.operand_record(q_p, mo.ROWS) is None and mo.operand_record(q_p, mo.SECOND) is None
    q_p.add_(1)
    assert mo.operand_record(q, mo.ROWS) is None and mo.format_of(q) is None
    q2, s2, _, _ = _tagged((2, 3, 4, 8))
    q2_p, s2_p = q2.permute(0, 3, 1, 2), s2.permute(0, 3, 1, 2)
    mo.carry(q2, s2, q2_p, s2_p)
    q2.add_(1)
    assert mo.operand_record(q2_p, mo.NHWC) is None and mo.format_of(q2_p) is None


def test_carry_of_a_stale_or_bare_source_carries_nothing():
    q, s, _, _ = _tagged((2, 4, 8))
    q.add_(1), s.mul_(2)
    q_t, s_t = q.transpose(-1, -2), s.transpose(-1, -2)
    assert mo.carry(q, s, q_t, s_t) is None
    assert mo.format_of(q_t) is None and not mo.is_pow2(s_t) and mo.operand_record(q_t, mo.SECOND) is None
    # format and flag without an operand (a row that is no whole number of 16-byte chunks): those two still travel
    q, s = mo.set_format(torch.zeros(2, 4, 8), "fp6_e2m3"), mo.set_pow2(torch.ones(2, 4, 1))
    q_t, s_t = q.transpose(-1, -2), s.transpose(-1, -2)
    assert mo.carry(q, s, q_t, s_t) is None and mo.format_of(q_t) == "fp6_e2m3" and mo.is_pow2(s_t)


# ---- the copy ----------------------------------------------------------------------------------------------------------------------
def test_copy_hints_restamps_for_the_clone():
    q, s, _, _ = _tagged((4, 64))
    q.add_(0)                                                       # the source's counter is no longer the clone's
    mo.quantized(q, s, "fp8_e4m3")
    table = get_quantization_map("fp8_e4m3")
    for src, read, want in ((q, mo.format_of, "fp8_e4m3"), (s, mo.is_pow2, True), (table, mo.map_name, "fp8_e4m3")):
        dst = src.clone().detach()
        assert read(dst) in (None, False)
        assert mo.copy_hints(src, dst) is dst and read(dst) == want and dst._qt_mx_ver == dst._version == 0
    assert mo.operand_record(mo.copy_hints(_tagged((4, 64))[0], torch.zeros(4, 64)), mo.ROWS) is None       # the operand stays behind
    stale = _tagged((4, 64))[0].add_(1)
    assert mo.format_of(mo.copy_hints(stale, stale.clone())) is None


# ---- the map tag -------------------------------------------------------------------------------------------------------------------
def test_map_tag_is_versioned():
    m = torch.zeros(65536, dtype=torch.bfloat16)
    assert mo.map_name(m) is None
    assert mo.tag_map(m, "posit8_1") is m and mo.map_name(m) == "posit8_1" and m._qt_mx_ver == m._version
    m.add_(1)
    assert mo.map_name(m) is None
    # "no format" is a tag as well (pt2e_native fuses the dequantize behind a GEMM when its output map is that identity)
    assert mo.map_name(mo.tag_map(m, None)) == "None" and mo.map_name(get_quantization_map(None)) == "None"


def test_package_tables_come_tagged_with_a_version():
    table = get_quantization_map("fp8_e4m3")
    assert mo.map_name(table) == "fp8_e4m3" and table._qt_mx_ver == table._version
    flat = _table_for("nf4", None)                                  # a NormalFloat (indices, values) pair as one flat table
    assert flat.shape == (65536,) and mo.map_name(flat) == "nf4" and flat._qt_mx_ver == flat._version


def test_format_of_qmap_by_tag_then_once_by_content():
    table = get_quantization_map("fp4_e2m1")
    assert mo.format_of_qmap(table) == "fp4_e2m1"
    copy = table.clone()                                            # what `model.to()` or a state dict leaves: no tag
    assert mo.map_name(copy) is None and mo.format_of_qmap(copy) == "fp4_e2m1" and mo.map_name(copy) == "fp4_e2m1"
    other = get_quantization_map("int8").clone()
    assert mo.format_of_qmap(other) is None and mo.map_name(other) == ""          # looked at: not asked again
    assert mo.format_of_qmap(get_quantization_map("int8")) is None
    copy.zero_()                                                    # a written-to map is looked at again
    assert mo.map_name(copy) is None and mo.format_of_qmap(copy) is None


# ---- the weight cache --------------------------------------------------------------------------------------------------------------
class _CountingPack:
    """Stands in for the packer: takes the formats in `takes`, counts every call."""

    def __init__(self, takes):
        self.takes, self.calls = takes, []

    def __call__(self, w, s, fid, block_size):
        self.calls.append(fid)
        return (torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8)) if fid in self.takes else None


@pytest.mark.parametrize("slot", [mo.GEMM_SLOT, mo.CONV_SLOT])
def test_weight_cache(slot):
    w, s = torch.zeros(8, 64, dtype=torch.bfloat16), torch.ones(8, 2, dtype=torch.bfloat16)
    pack = _CountingPack({0})

    def get(scale=s, bs=32, extent=64):
        return mo.weight_operand(w, scale, bs, slot, lambda: (w, scale), extent, pack)

    first = get()
    assert first[0] == 0 and pack.calls == [4, 2, 3, 0]             # narrow first, up to the first format the packer takes
    assert get() is first and len(pack.calls) == 4                  # unchanged weight and scale: nothing is packed
    for n, change in enumerate((lambda: w.add_(0), lambda: s.add_(0))):
        change()
        assert get() is not first and len(pack.calls) == 4 * (n + 2)
    assert get(bs=64) is not None and len(pack.calls) == 16         # another block size
    assert get(scale=s.clone()) is not None and len(pack.calls) == 20      # another scale tensor
    assert getattr(w, slot)[1][0] == 0
    # the other slot is another cache
    assert getattr(w, mo.CONV_SLOT if slot == mo.GEMM_SLOT else mo.GEMM_SLOT, None) is None


def test_weight_cache_refusal_known_format_and_row_rule():
    w, s = torch.zeros(8, 64, dtype=torch.bfloat16), torch.ones(8, 2, dtype=torch.bfloat16)
    refuse = _CountingPack(set())
    assert mo.weight_operand(w, s, 32, mo.GEMM_SLOT, lambda: (w, s), 64, refuse) is None and refuse.calls == [4, 2, 3, 0, 1]
    assert mo.weight_operand(w, s, 32, mo.GEMM_SLOT, lambda: (w, s), 64, refuse) is None and len(refuse.calls) == 5      # cached as None
    mo.set_format(w, "fp8_e5m2")                                    # not a write to the weight: the cached refusal stands
    assert mo.weight_operand(w, s, 32, mo.GEMM_SLOT, lambda: (w, s), 64, refuse) is None and len(refuse.calls) == 5
    w2 = mo.set_format(torch.zeros(8, 64, dtype=torch.bfloat16), "fp8_e5m2")
    alone = _CountingPack({0, 1, 4})
    assert mo.weight_operand(w2, s, 32, mo.GEMM_SLOT, lambda: (w2, s), 64, alone)[0] == 1 and alone.calls == [1]        # tried alone
    w3 = mo.set_format(torch.zeros(8, 64, dtype=torch.bfloat16), "int8")
    anyf = _CountingPack({3})
    assert mo.weight_operand(w3, s, 32, mo.GEMM_SLOT, lambda: (w3, s), 64, anyf)[0] == 3 and anyf.calls == [4, 2, 3]
    # the 16-byte rule is applied to the extent the caller names: 32 elements of a 6-bit format are 24 bytes
    w4 = torch.zeros(8, 32, 3, 3, dtype=torch.bfloat16)
    six = _CountingPack({2, 3, 0})
    assert mo.weight_operand(w4, s, 32, mo.CONV_SLOT, lambda: (w4.view(8, -1), s), 32, six)[0] == 0 and six.calls == [4, 0]


def test_the_two_callers_share_the_cache(monkeypatch):
    from quantized_training import mx_conv, mx_gemm
    seen = []

    def pack_rows(w, s, fid, block_size):
        seen.append((tuple(w.shape), tuple(s.shape), fid, block_size))
        return torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8)
    monkeypatch.setattr(mx_gemm, "_pack_rows", pack_rows)
    monkeypatch.setattr(mx_conv, "_pack_rows", pack_rows)
    w, s = torch.zeros(8, 64, dtype=torch.bfloat16), torch.ones(8, 2, dtype=torch.bfloat16)
    assert mx_gemm._weight_operand(w, s, 32)[0] == 4 and mx_gemm._weight_operand(w, s, 32)[0] == 4
    wc, sc = torch.zeros(8, 64, 3, 2, dtype=torch.bfloat16), torch.ones(8, 2, 3, 2, dtype=torch.bfloat16)
    assert mx_conv._conv_weight_operand(wc, sc, 32)[0] == 4 and mx_conv._conv_weight_operand(wc, sc, 32)[0] == 4
    assert seen == [((8, 64), (8, 2), 4, 32), ((8, 384), (8, 12), 4, 32)]


# ---- inference tensors -------------------------------------------------------------------------------------------------------------
def test_inference_tensors_are_untracked_and_always_valid():
    with torch.inference_mode():
        q, s, codes, e8 = _tagged((2, 4, 8))
        assert q.is_inference()
        with pytest.raises(RuntimeError):
            q._version
        assert mo.format_of(q) == "fp8_e4m3" and mo.is_pow2(s) and mo.operand(q, mo.ROWS, 0, 32, 8, 8)[0] is codes
        q_t, s_t = q.transpose(-1, -2), s.transpose(-1, -2)
        assert mo.carry(q, s, q_t, s_t) == mo.SECOND and mo.operand_record(q_t, mo.SECOND)[2] is codes
        dst = mo.copy_hints(q, q.clone())
        assert mo.format_of(dst) == "fp8_e4m3"
        m = mo.tag_map(torch.zeros(4), "x")
        assert mo.map_name(m) == "x"
        q.add_(1)                                                   # staleness cannot be seen here: the record still reads
        assert mo.format_of(q) == "fp8_e4m3"
        assert mo.drop_operand(q) is q and mo.operand_record(q, mo.ROWS) is None
    assert mo.format_of(q) == "fp8_e4m3" and q._qt_mx_ver == "untracked"          # and outside the mode as well
