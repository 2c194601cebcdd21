"""Golden fixture of upstream's PT2E flow on a block-scaled CNN -- run by hand in the container that holds the upstream checkout
(`python tests/golden/gen_golden_mx_conv.py`, imports it through _ref_import); tests/test_conv_mx_cpu.py imports only the model and
input helpers below and runs them against this package.

  pt2e_mx_conv.npz + pt2e_mx_conv.json
        conv(3 -> 32, 3 x 3) -> relu -> conv(32 -> 64, 3 x 3, stride 2, padding 1) -> relu -> conv(64 -> 64, 1 x 1) in fp32 on the CPU
        through upstream's prepare_pt2e / two calibration calls / convert_pt2e with `fp8_e4m3,qs=microscaling,bs=32` activations and
        weights and power-of-two scales: the prepared output, the converted graph's rows, kwargs and node dtypes (conv2d_mx with a
        quantize along axis 1 in front of it, quantize_pt2e.py::_mx_op_mapping), its weight / scale buffers and its output.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
KW = dict(input_activation="fp8_e4m3,qs=microscaling,bs=32", weight="fp8_e4m3,qs=microscaling,bs=32", force_scale_power_of_two=True)


class ToyCNN(nn.Module):
    def __init__(self):
        super().__init__()
        self.c1 = nn.Conv2d(3, 32, 3)
        self.c2 = nn.Conv2d(32, 64, 3, stride=2, padding=1)
        self.c3 = nn.Conv2d(64, 64, 1)

    def forward(self, x):
        return self.c3(torch.relu(self.c2(torch.relu(self.c1(x)))))


def model():
    m = ToyCNN().eval()
    r = np.random.default_rng(5)
    with torch.no_grad():
        for _, p in sorted(m.named_parameters()):
            p.copy_(torch.from_numpy((r.standard_normal(tuple(p.shape)) * 0.2).astype(np.float32)))
    return m


def inputs():
    r = np.random.default_rng(29)
    return [torch.from_numpy((r.standard_normal((2, 3, 12, 10)) * (i + 1)).astype(np.float32)) for i in range(2)]


def bits32(t):
    b = t.detach().float().contiguous().view(torch.int32).numpy().astype(np.uint32)
    b[((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)] = 0x7FC00000
    return b


def graph_rows(gm):
    def nm(a):
        if isinstance(a, torch.fx.Node):
            return a.name
        if isinstance(a, (list, tuple)):
            return [nm(x) for x in a]
        return a if isinstance(a, (int, float, str, bool, type(None))) else str(a)
    return [[n.op, n.name, str(n.target), nm(list(n.args))] for n in gm.graph.nodes]


def record(qp):
    """The flow on `qp` (upstream's quantize_pt2e here, this package's in the test) -> (arrays, info)."""
    xs = inputs()
    gm = qp.prepare_pt2e(model(), qp.get_default_quantizer(**KW), (xs[0],))
    arrays, info = {}, {"kw": KW, "prepared_graph": graph_rows(gm)}
    with torch.no_grad():
        gm(xs[0])
        arrays["y_prepared"] = bits32(gm(xs[1]))
    gc = qp.convert_pt2e(gm)
    info["converted_graph"] = graph_rows(gc)
    info["converted_kwargs"] = {n.name: {k: (v.name if isinstance(v, torch.fx.Node) else v) for k, v in n.kwargs.items()}
                                for n in gc.graph.nodes if n.kwargs}
    info["node_dtype"] = {n.name: (list(n.meta["dtype"]) if isinstance(n.meta["dtype"], tuple) else n.meta["dtype"])
                          for n in gc.graph.nodes if n.meta.get("dtype") is not None}
    info["buffers"] = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in gc.named_buffers()}
    for k, v in gc.named_buffers():
        arrays["buf__" + k] = bits32(v)
    with torch.no_grad():
        arrays["y_converted"] = bits32(gc(xs[1]))
    return arrays, info


def main():
    sys.path.insert(0, HERE)
    from _ref_import import load_reference
    ref = load_reference(with_quantize=True)
    assert ref.quantize_pt2e is not None, getattr(ref, "pt2e_error", None)
    arrays, info = record(ref.quantize_pt2e)
    targets = [row[2] for row in info["converted_graph"]]
    assert sum("conv2d_mx" in t for t in targets) == 3, targets
    np.savez_compressed(os.path.join(HERE, "pt2e_mx_conv.npz"), **arrays)
    with open(os.path.join(HERE, "pt2e_mx_conv.json"), "w") as f:
        json.dump(info, f, indent=1)
    print("wrote pt2e_mx_conv.npz / .json:", len(arrays), "arrays,", len(info["converted_graph"]), "graph rows")


if __name__ == "__main__":
    main()
