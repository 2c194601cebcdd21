"""Host side of the in-tree Conv2d backward (csrc/qt_conv_backward.hip, conv_route.py): the QT_CONV_GEMM=auto rules of the two backward
products pinned on the shape classes of tools/exp_conv2d_backward.py, the plan's arithmetic (no device needed), the README row and
the library's exports.  The device side is tests/test_gpu_conv_backward.py."""
import ctypes
import os
import re

from quantized_training import _native, conv_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H = W, Cin, Cout, k) at batch 32, stride 1, padding k // 2: the rows of profiles/conv2d_bwd_routes.txt
TABLE_3X3 = [(56, 64, 64, 3), (28, 128, 128, 3), (14, 256, 256, 3), (7, 512, 512, 3)]
TABLE_1X1 = [(56, 64, 64, 1), (56, 64, 256, 1), (56, 256, 64, 1), (28, 128, 512, 1), (28, 512, 128, 1), (14, 256, 1024, 1), (14, 1024, 256, 1),
             (7, 512, 2048, 1), (7, 2048, 512, 1)]


def _ints(hw, cin, cout, k):
    return (32, hw, hw, cin, cout, k, k, 1, 1, k // 2, k // 2, 1, 1)


def _auto(hw, cin, cout, k):
    """(dgrad, wgrad) of the auto rules on a table row, through the plan the route itself consults (256 CUs without a device)."""
    d, g = conv_route.backward_plan(*_ints(hw, cin, cout, k))
    assert d.taken and g.taken
    return (conv_route._auto_takes_dgrad(32 * hw * hw, cin, d.k_tiles), conv_route._auto_takes_wgrad(32 * hw * hw, cout, k * k * cin, g.ksplit))


TABLE = os.path.join(ROOT, "profiles", "conv2d_bwd_routes.txt")

# what the committed rules give each shape class of the table: (dgrad, wgrad)
PINNED = {s: (False, False) for s in TABLE_3X3 + TABLE_1X1}


def test_auto_rules_pinned():
    for shape, routes in PINNED.items():
        assert _auto(*shape) == routes, shape
    # functions of the shape alone: the same answer whatever the switch says
    os.environ["QT_CONV_GEMM"] = "1"
    try:
        assert _auto(56, 64, 64, 3) == PINNED[(56, 64, 64, 3)]
    finally:
        del os.environ["QT_CONV_GEMM"]


def test_a_product_goes_in_tree_only_where_the_committed_table_measured_it_faster():
    """A rule may send a shape class in-tree only on the strength of the committed table: its row must exist, name the same route,
    and show the kernel faster than the library by more than the spread the table states for the library."""
    if not any(d or w for d, w in PINNED.values()):
        return                                                         # every class stays with the library: nothing to back up
    table = open(TABLE).read()
    rows = [ln for ln in table.splitlines() if ln and not ln.startswith("#")]
    assert len(rows) == len(TABLE_3X3) + len(TABLE_1X1)
    spread = float(re.search(r"largest run-to-run spread.*?([0-9.]+) %", table).group(1)) / 100
    for (hw, cin, cout, k), row in zip(TABLE_3X3 + TABLE_1X1, rows):
        assert row.startswith(f"32x{cin}x{hw}x{hw} -> {cout} {k}x{k} "), row
        d, w = PINNED[(hw, cin, cout, k)]
        assert re.findall(r"auto -> (in-tree|library)", row) == ["in-tree" if d else "library", "in-tree" if w else "library"], (row, d, w)
        rd = float(re.search(r"library / \(in-tree \+ copy\)\s+([0-9.]+)", row).group(1))
        rw = float(re.search(r"library / in-tree\s+([0-9.]+)", row).group(1))
        assert (not d or rd > 1.0 + spread) and (not w or rw > 1.0 + spread), row


def test_backward_plan_arithmetic_without_a_device():
    d, g = conv_route.backward_plan(*_ints(56, 64, 64, 3))
    assert (d.tile_m, d.tile_n, d.tiles_m, d.tiles_n, d.k_tiles, d.ksplit) == (128, 64, 784, 1, 9, 1)
    assert (g.tile_m, g.tile_n, g.tiles_m, g.tiles_n, g.k_tiles) == (64, 64, 1, 9, 1568)
    assert g.ksplit > 1 and g.ws_bytes == 9 * g.ksplit * 64 * 64 * 4 and g.n_tickets == 9
    assert conv_route.backward_plan(32, 56, 56, 3, 64, 3, 3, 1, 1, 1, 1, 1, 1) is None          # the stem
    assert conv_route.backward_plan(32, 56, 56, 64, 12, 3, 3, 1, 1, 1, 1, 1, 1) is None         # Cout % 8
    assert conv_route._backward_routes("1", 32, 56, 56, 64, 64, 3, 3, (1, 1), (1, 1), (1, 1)) == (True, True)
    assert conv_route._backward_routes("1", 32, 56, 56, 64, 12, 3, 3, (1, 1), (1, 1), (1, 1)) == (False, False)


def test_readme_row_and_exports():
    readme = open(os.path.join(ROOT, "README.md")).read()
    row = [ln for ln in readme.splitlines() if ln.startswith("| `QT_CONV_GEMM=auto/0/1`")]
    assert len(row) == 1 and "backward" in row[0] and "qt_conv2d_dgrad_bf16" in row[0] and "qt_conv2d_wgrad_bf16" in row[0]
    L = _native.lib()
    assert L.qt_abi_version() == 3
    for name in ("qt_conv2d_dgrad_bf16", "qt_conv2d_wgrad_bf16", "qt_conv2d_backward_plan"):
        assert hasattr(L, name) and name in _native.SIGNATURES
    assert ctypes.sizeof(_native.QtConv2dProductPlan) == 7 * 4 + 4 + 2 * ctypes.sizeof(ctypes.c_size_t)
