"""conv2d_mx on the integer matrix cores (qt_conv2d_mxi), the parts that need no GPU: the entry point and its declaration, what the
router answers for CPU tensors, the committed route rule against every row of the table it was read off, and the composite on the CPU."""
import os
import re

import pytest
import torch

from quantized_training import _native, mx_conv, mx_gemm, mx_operand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = re.compile(r"^(bf16|fp32) int6 x \S+ \S+ -> \d+ (\d)x\d \| m (\d+) cout (\d+) k (\d+) \| native \+ pack +([\d.]+) us .*\| composite +([\d.]+) us "
                 r"\(spread +([\d.]+) %\).*\| bar (cleared|missed) \| rule -> (native|composite) ")


def test_symbol_is_exported_and_declared():
    assert hasattr(_native.lib(), "qt_conv2d_mxi") and len(_native.SIGNATURES["qt_conv2d_mxi"][1]) == 22 and _native.lib().qt_abi_version() == 3
    decl = re.search(r"int qt_conv2d_mxi\(([^;]*)\);", open(os.path.join(ROOT, "include", "qt_hip.h")).read())
    assert decl is not None and len(decl.group(1).split(",")) == 22


def test_route_rule_against_every_row_of_the_committed_table():
    """profiles/conv2d_mxi.txt: the rule lists a class only where the native median beat the composite's by more than its spread."""
    rows = [ROW.match(line) for line in open(os.path.join(ROOT, "profiles", "conv2d_mxi.txt")) if not line.startswith("#")]
    assert len(rows) == 52 and all(rows), "13 layers x 2 dtypes x 2 weight formats"
    for r in rows:
        (kf, m, cout, k), (tn, tc, sc) = map(int, r.group(2, 3, 4, 5)), map(float, r.group(6, 7, 8))
        cleared = tn < tc * (1.0 - sc / 100.0)
        takes = mx_conv._int_conv_route_takes(m, cout, k, kf * kf, torch.bfloat16 if r.group(1) == "bf16" else torch.float32)
        assert (r.group(9) == "cleared") == cleared and (r.group(10) == "native") == takes and (cleared or not takes), r.group(0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("code", [False, True], ids=["int6 x int6", "int6 x codebook"])
def test_cpu_tensors_are_nobodys_candidate_and_run_the_composite(code, dtype, monkeypatch):
    """Neither family looks at a CPU tensor: no library call, nothing counted, the reference's composite bit for bit."""
    g = torch.Generator().manual_seed(0)
    x, w = torch.randint(-31, 32, (2, 64, 6, 5), generator=g).to(dtype), torch.randint(0 if code else -31, 16 if code else 32, (8, 64, 3, 3), generator=g).to(dtype)
    xs, ws = (torch.rand(2, 1, 6, 5, generator=g) + 0.5).to(dtype), (torch.rand(8, 1, 3, 3, generator=g) + 0.5).to(dtype)
    for t in (x,) if code else (x, w):
        mx_operand.set_format(t, "int6")
    wc = torch.arange(-8.0, 8.0).to(dtype) if code else None
    monkeypatch.setattr(mx_conv._native, "lib", lambda: pytest.fail("the library was called"))
    args = (x, w, None, (1, 1), (1, 1), (1, 1), 1, xs, ws, 64, None, wc)
    mx_gemm.STATS.reset()
    assert mx_conv._int_conv2d(*args) is None and mx_conv._float_conv2d(*args) is None and mx_conv.mx_conv2d_or_none(*args) is None
    got = torch.ops.quantized_ops.conv2d_mx(x, w, None, [1, 1], [1, 1], [1, 1], 1, input_scale=xs, weight_scale=ws, block_size=64, weight_code=wc)
    want = torch.nn.functional.conv2d(x * xs.repeat_interleave(64, 1), (wc[w.to(torch.long)].to(dtype) if code else w) * ws.repeat_interleave(64, 1), None, 1, 1, 1)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert got.dtype == want.dtype and torch.equal(got.view(bits), want.view(bits)) and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 0)
