"""The split of K of the native int8 convolution without a GPU: the new symbols, the host-only plan and its properties, the refusals
the *_ws entry points answer before any device call, the committed rule against the rows of profiles/conv2d_q_splitk.txt, and the
opt-in: the mark fuse_native_gemms(split_k=True) leaves on the codes buffers, what _conv_q_decline and the chain pass make of it."""
import ctypes
import os
import re

import torch

import conv_q_splitk_cases as C
from quantized_training import _native, pt2e_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_Q, CONV_QC = "quantized_ops.conv2d_q.default", "quantized_ops.conv2d_qc.default"
WS_TAIL = ["ksplit", "ws", "ws_bytes", "tickets", "n_tickets", "stream"]


def test_entry_points_are_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(ROOT, "include", "qt_hip.h")).read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name, sibling in (("qt_q8_conv2d_ws", "qt_q8_conv2d"), ("qt_q8_conv2d_codes_ws", "qt_q8_conv2d_codes")):
        decl = re.search(r"\bint\s+" + name + r"\(([^;]*?)\);", header, re.S)
        assert decl is not None and name in _native.SIGNATURES
        args = [a.strip() for a in decl.group(1).split(",") if a.strip()]
        assert len(args) == len(_native.SIGNATURES[name][1]) == len(_native.SIGNATURES[sibling][1]) + 5, name
        assert [a.split()[-1].lstrip("*") for a in args[-6:]] == WS_TAIL
        assert _native.SIGNATURES[name][1][:-6] == _native.SIGNATURES[sibling][1][:-1]          # the sibling's leading arguments
        getattr(lib, name)
    assert re.search(r"\bint\s+qt_q8_conv2d_plan\(long M, int Cout, int K, int \*ksplit, size_t \*ws_bytes, size_t \*n_tickets\);", header)
    assert len(_native.SIGNATURES["qt_q8_conv2d_plan"][1]) == 6
    getattr(lib, "qt_q8_conv2d_plan")
    assert _native.lib().qt_abi_version() == 3
    assert pt2e_native.STATS["conv2d_split_k"] >= 0


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def test_plan_properties():
    """S = 1 once the tiles fill the CU count; 1 <= S <= nk; a split only where S workgroups per tile still fit the chip; workspace
    bytes and tickets follow from S and the tile count; the same answer on every call."""
    cus = cu_count()
    split_somewhere = False
    for m in (1, 25, 128, 129, 392, 1568, 6272, 25088, 128 * cus, 128 * cus + 1, 100352):
        for cout in (16, 64, 128, 144, 512):
            for k in (32, 128, 256, 288, 1024, 2048, 4608, (1 << 17) - 32):
                s, wb, nt = _native.q8_conv_plan(m, cout, k)
                tiles, nk = -(-m // 128) * -(-cout // 128), -(-k // 128)
                assert 1 <= s <= nk, (m, cout, k, s)
                assert tiles < cus or s == 1, (m, cout, k, s)
                assert s == 1 or tiles * s <= cus, (m, cout, k, s)
                assert (wb, nt) == ((tiles * s * C.SLAB, tiles) if s > 1 else (0, 0)), (m, cout, k, s)
                assert (s, wb, nt) == _native.q8_conv_plan(m, cout, k)
                split_somewhere |= s > 1
    assert split_somewhere
    assert _native.q8_conv_plan(0, 64, 256) == (1, 0, 0) and _native.q8_conv_plan(64, 0, 256) == (1, 0, 0)
    L = _native.lib()
    for bad in ((-1, 64, 256), (64, -1, 256), (64, 64, 0), (64, 64, 48), (64, 64, 1 << 17)):
        assert L.qt_q8_conv2d_plan(*bad, None, None, None) == _native.QT_ERR_BAD_ARG
    assert L.qt_q8_conv2d_plan(64, 64, 256, None, None, None) == 0


def test_ws_entry_points_answer_their_declines_before_any_device_call():
    L = _native.lib()
    buf = ctypes.create_string_buffer(1 << 18)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    BAD, UNAL = _native.QT_ERR_BAD_ARG, _native.QT_ERR_UNALIGNED

    def conv(ksplit=2, ws=p, wsb=2 * C.SLAB, tk=p, ntk=1, cin=256, x=p, n=1, codes=False):
        head = (x, p, p, 1, None, None, 0, 0, n, 4, 4, cin, 16, 1, 1, 1, 1, 0, 0, 1, 1)
        if codes:
            return L.qt_q8_conv2d_codes_ws(*head, 1, 0.0, 6.0, p, p, ksplit, ws, wsb, tk, ntk, None)
        return L.qt_q8_conv2d_ws(*head, ksplit, ws, wsb, tk, ntk, None)
    for codes in (False, True):
        assert conv(ws=None, codes=codes) == BAD and conv(tk=None, codes=codes) == BAD
        assert conv(wsb=2 * C.SLAB - 1, codes=codes) == BAD and conv(ntk=0, codes=codes) == BAD
        assert conv(ws=p + 8, codes=codes) == UNAL and conv(tk=p + 2, codes=codes) == UNAL
        assert conv(ksplit=3, codes=codes) == BAD and conv(ksplit=-1, codes=codes) == BAD and conv(cin=128, codes=codes) == BAD
        assert conv(cin=48, codes=codes) == BAD and conv(x=p + 4, codes=codes) == UNAL and conv(x=None, codes=codes) == BAD
        assert conv(n=0, codes=codes) == 0 and conv(n=0, ws=None, codes=codes) == 0               # empty: no launch
    del buf


# ---- the committed rule and the plan against the committed table ----------------------------------------------------------------
def table():
    """(m, cin, cout, kh, kw, nk, {S: that split clears the bar}) of every row of profiles/conv2d_q_splitk.txt (S = 1: the unsplit kernel)."""
    rows = []
    for line in open(os.path.join(ROOT, "profiles", "conv2d_q_splitk.txt")):
        m = re.match(r"(\d+)x(\d+)x(\d+)x(\d+) -> (\d+) (\d+)x(\d+) \| tiles (\d+) nk (\d+) .*?\| clears the bar: ((?:S=\d+:(?:yes|no) ?)+)\|", line)
        if m:
            n, cin, h, w, cout, kh, kw, tiles, nk = (int(v) for v in m.groups()[:9])
            assert tiles == -(-n * h * w // 128) * -(-cout // 128) and nk == -(-kh * kw * cin // 128)
            verdict = {int(s): v == "yes" for s, v in re.findall(r"S=(\d+):(yes|no)", m.group(10))}
            rows.append((n * h * w, cin, cout, kh, kw, nk, verdict))
    return rows


def test_split_route_rule_follows_the_committed_table():
    """The table covers the issue's seventeen rows, each with the unsplit kernel and every candidate split the shape admits.  A class
    the rule lists holds only measured rows on which the split the committed plan chooses (on a 256-CU device, the one measured)
    cleared the bar; the plan chooses only splits that were measured."""
    rows = table()
    assert len(rows) == 17
    for m, cin, cout, kh, kw, nk, verdict in rows:
        assert 1 in verdict and all(s <= nk for s in verdict)
        takes = pt2e_native._conv_q_split_route_takes(m, cout, cin, kh, kw)
        if cu_count() == 256:
            s = _native.q8_conv_plan(m, cout, kh * kw * cin)[0]
            assert s in verdict, f"the plan splits {m} x {cout} x {cin} {kh}x{kw} by {s}, which was not measured"
            assert not takes or verdict[s], f"the rule lists {m} x {cout} x {cin} {kh}x{kw}, which did not clear the bar at S = {s}"
        else:
            assert not takes or any(verdict.values())
    # outside the table nothing is listed: a shape no row is near
    assert not pt2e_native._conv_q_split_route_takes(7, 8, 32, 1, 1)


# ---- the opt-in ---------------------------------------------------------------------------------------------------------------------
def marks(gm):
    return {name: pt2e_native._split_k_marked(buf) for name, buf in gm.named_buffers() if name.endswith("_codes")}


def test_pass_marks_buffers_only_under_split_k(monkeypatch):
    """The default conversion and split_k=False leave the graph and its buffers as they are today (no attribute); split_k=True gives
    the same graph, node for node, and marks the codes buffers of the two gather layers."""
    default, x = C.convert_project_net(monkeypatch, "cpu", native=True)
    off, _ = C.convert_project_net(monkeypatch, "cpu", native=True, split_k=False)
    on, _ = C.convert_project_net(monkeypatch, "cpu", native=True, split_k=True)
    rows = lambda gm: [(n.op, str(n.target), tuple(str(a) for a in n.args)) for n in gm.graph.nodes]  # noqa: E731
    assert rows(default) == rows(off) == rows(on) and C.call_targets(on).count(CONV_Q) == 2
    assert marks(default) == marks(off) == {"expand_weight_codes": False, "project_weight_codes": False, "fc_weight_codes": False}
    assert not any(hasattr(b, "_qt_split_k") for gm in (default, off) for b in gm.buffers())
    assert marks(on) == {"expand_weight_codes": True, "project_weight_codes": True, "fc_weight_codes": False}      # the Linear: not a gather layer
    upstream, _ = C.convert_project_net(monkeypatch, "cpu", native=False, split_k=True)                 # without native fusion: nothing
    assert CONV_Q not in C.call_targets(upstream) and not any(hasattr(b, "_qt_split_k") for b in upstream.buffers())
    with torch.no_grad():
        assert torch.equal(default(x), on(x))
    moved = on.project_weight_codes.clone()                                                           # a copy loses the mark
    assert not pt2e_native._split_k_marked(moved)


def decline(weight_codes, cin=1024, cout=32):
    x = pt2e_native._Operand((4, cin, 10, 10), torch.bfloat16, "cpu")
    s, qmap = pt2e_native._Operand((1,), torch.bfloat16, "cpu"), pt2e_native._Operand((65536,), torch.bfloat16, "cpu")
    return pt2e_native._conv_q_decline(x, s, qmap, weight_codes, None, [1, 1], [0, 0], [1, 1], 1, torch.ones(1, dtype=torch.bfloat16), "int8",
                                       on_device=True)


def test_decline_with_and_without_the_mark(monkeypatch):
    """A reducing 1 x 1 layer (1024 -> 32 over 400 pixels) under the committed rules: unmarked, the parent's reason, whatever the
    split rule says; marked, the split rule decides; with the rules bypassed both are taken."""
    plain = torch.zeros(32, 1, 1, 1024, dtype=torch.int8)
    marked = pt2e_native.mark_split_k(plain.clone())
    assert not pt2e_native._conv_q_route_takes(400, 32, 1024, 1, 1)
    for split_rule in (True, False):
        monkeypatch.setattr(pt2e_native, "_conv_q_split_route_takes", lambda *a, r=split_rule: r)
        assert decline(plain) == "route rule: profiles/conv2d_q.txt"
        assert decline(marked) == (None if split_rule else "split-K route rule: profiles/conv2d_q_splitk.txt")
    seen = []
    monkeypatch.setattr(pt2e_native, "_conv_q_split_route_takes", lambda *a: seen.append(a) or True)
    assert decline(marked) is None and seen == [(400, 32, 1024, 1, 1)]
    monkeypatch.setattr(pt2e_native, "_conv_q_route_takes", lambda *a: True)                             # a layer the old rule takes
    seen.clear()
    assert decline(marked) is None and decline(plain) is None and seen == []
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    monkeypatch.setattr(pt2e_native, "_conv_q_route_takes", lambda *a: False)
    monkeypatch.setattr(pt2e_native, "_conv_q_split_route_takes", lambda *a: False)
    assert decline(marked) is None and decline(plain) is None


def test_chain_pass_takes_the_projecting_edge_only_with_the_mark(monkeypatch):
    """The committed-rule path of fuse_conv_q_chains, with a rule that takes expanding layers and a split rule that takes marked
    reducing ones: the edge expand -> relu -> project is rewritten only in the graph converted with split_k=True."""
    monkeypatch.setattr(pt2e_native, "_conv_q_route_takes", lambda m, cout, cin, kh, kw: cout >= cin)
    monkeypatch.setattr(pt2e_native, "_conv_q_split_route_takes", lambda *a: True)
    plain, x = C.convert_project_net(monkeypatch, "cpu", native=True)
    assert pt2e_native.fuse_conv_q_chains(plain) == 0 and CONV_QC not in C.call_targets(plain)
    both, _ = C.convert_project_net(monkeypatch, "cpu", native=True, split_k=True, chain_convs=True)
    t = C.call_targets(both)
    assert t.count(CONV_QC) == 2 and t.count(CONV_Q) == 0
    with torch.no_grad():
        assert torch.equal(plain(x), both(x))
