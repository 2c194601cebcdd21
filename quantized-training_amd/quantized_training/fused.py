"""Routing of the fake-quant GEMMs: the QAT Linear's fused kernels (qt_linear_fq8_bf16, qt_linear_fqt_bf16, qt_linear_fq_bf16), the gated
MLP's one-launch front half, sibling groups that share a launch, the library FP8 GEMM (lt_fp8_gemm), and what ran (ROUTES,
routes_report).  The attention core's routing is attention_route.py.

``fused_linear_or_none`` returns ``None`` whenever the fused HIP GEMM does not apply, and the
caller then runs the unfused sequence (HIP elementwise fake-quant + library GEMM); both are
device paths -- there is no CPU fallback for device tensors.
"""
import collections
import ctypes

import torch

from . import _native, handover, precomputed, switches
from .fake_quantize import STATS, FusedAmaxObsFakeQuantFunction, FusedAmaxObsFakeQuantize, _stream_ptr, launch_scale_update
from .quantizer.quantizer import QScheme

_IDENTITY = _native.QtFormat(_native.QT_FMT_IDENTITY, 0, 0, 0.0, 0.0)


def fused_gemm_enabled():
    return switches.on("QT_FUSED_GEMM")


def fp8_gemm_enabled():
    return switches.on("QT_FP8_GEMM")


def fq8_gemm_mode():
    """QT_FQ8_GEMM: "auto" (default) -- per problem shape, whichever of the two routes measured faster on its first call;
    "1" -- always the hand-written FP8 GEMM with the weight fake-quantizer in its operand path (qt_linear_fq8_bf16);
    "0" -- always the weight pass + library GEMM pair."""
    return switches.mode("QT_FQ8_GEMM")


def fq8_gemm_enabled():
    return fq8_gemm_mode() != "0"


_FQ8_CHOICE = {}          # (M, Ns, K, activation dtype, weight format, device) -> True: fused kernel, False: pass + library GEMM
ROUTES = {}               # what ran, for the bench line: "MxNxK" -> route name (first decision per shape)

# Measured on MI355X (tools/exp_linear_fq8.py, gpurun_out/fq8_routes.log -> profiles/r03_fq8_routes.txt): microseconds of the fused
# kernel against the weight pass + library GEMM, weights rotating beyond the Infinity Cache.  (M, sum N, K) -> fused kernel wins.
# The default route of a shape is this table, then the rule below: the same on every box, rank and run.
_FQ8_TABLE = {
    (1024, 11008, 4096): True,    # 54.7 / 69.1
    (1024, 4096, 11008): True,    # 68.0 / 72.8
    (1024, 4096, 4096): True,     # 27.9 / 32.9
    (1024, 12288, 4096): True,    # 54.7 / 70.5  (q / k / v)
    (1024, 32000, 4096): True,    # 159.8 / 169.8
    (1024, 8192, 4096): True,     # 44.9 / 50.2
    (1024, 6144, 4096): True,     # 40.7 / 43.1
    (512, 11008, 4096): True,     # 43.3 / 56.0
    (256, 11008, 4096): True,     # 30.0 / 43.2
    (2048, 11008, 4096): True,    # 102.5 / 105.3
    (2048, 4096, 4096): False,    # 45.5 / 45.0
    (4096, 4096, 4096): False,    # 87.6 / 57.6
    (6144, 768, 768): True,       # 16.7 / 27.2
    (6144, 2304, 768): False,     # 29.6 / 27.6  (q / k / v)
    (6144, 3072, 768): False,     # 35.2 / 30.1
    (6144, 768, 3072): False,     # 34.4 / 27.6
    (1024, 13824, 5120): False,   # 99.1 / 88.2
    (1024, 5120, 13824): False,   # 111.5 / 107.2
    (1024, 5120, 5120): True,     # 46.3 / 47.1
    (1024, 15360, 5120): False,   # 105.9 / 96.7 (q / k / v)
}


def _note_route(kind, M, ns, K, route):
    ROUTES.setdefault(f"{kind}:{M}x{sum(ns)}x{K}", route)


def routes_report():
    """The GEMM routes taken so far, per problem shape, and for library FP8 GEMMs which of the library's suggestions ran
    (bench.py puts them into its JSON line)."""
    out = dict(sorted(ROUTES.items()))
    out.update(sorted(LT_ALGOS.items()))
    from .modules.qat.linear import GEMM_ROUTES                # the training step's products (csrc/qt_train_gemm.hip or torch's GEMM)
    out.update(sorted(GEMM_ROUTES.items()))
    from .optim import ROUTES as OPT_ROUTES                    # clip_grad_norm_ + optimizer.step() (csrc/qt_optimizer.hip or torch's launches)
    out.update(sorted(OPT_ROUTES.items()))
    from .conv_route import CONV_ROUTES                        # QAT convolutions (csrc/qt_conv.hip or the library's convolution)
    out.update(sorted(CONV_ROUTES.items()))
    from .pt2e_native import GWA_ROUTES                        # packed group-wise affine Linears (csrc/qt_gwa_gemm.hip or dequantize + library GEMM)
    out.update(sorted(GWA_ROUTES.items()))
    return out


def _fq8_heuristic(M, ns, K, device):
    """Shapes the table does not list: the fused kernel where it fills the chip in one round of 256-row tiles at least five column
    groups wide -- what the sweep in DESIGN.md 6b showed for M <= 1024."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    tiles_m = (M + 255) // 256
    groups = sum(ns) // 16
    tn_min = (groups + 11) // 12
    if tiles_m * tn_min > cus or tiles_m > cus:
        return False
    nt = groups / max(1, cus // tiles_m)
    return M <= 1024 and nt >= 5.0 and K <= 8192


def fq8_route_is_fused(x8, layers):
    """Route of one fake-quant Linear problem (x8 [M, K] FP8 codes x the bf16 weights of `layers`): QT_FQ8_GEMM=0 / 1 forces it; else
    the committed table, else the closed-form rule.  Never a measurement: a timing race would make the summation order -- and so
    the logits -- depend on the box, the run and the rank, and a lazily measured choice would need a collective that not every rank
    reaches (windows are dealt round-robin)."""
    K = x8.shape[-1]
    M = x8.numel() // K
    ns = tuple(l.weight.shape[0] for l in layers)
    mode = fq8_gemm_mode()
    if mode != "auto":
        hit = mode == "1"
    else:
        hit = _FQ8_TABLE.get((M, sum(ns), K))
        if hit is None:
            key = (M, ns, K, x8.dtype, layers[0].weight_fake_quant._qt_format.key(), x8.device.index)
            hit = _FQ8_CHOICE.get(key)
            if hit is None:
                hit = _FQ8_CHOICE[key] = _fq8_heuristic(M, ns, K, x8.device)
    _note_route("fq8", M, ns, K, "fused_fp8_gemm" if hit else "weight_pass+library_fp8_gemm")
    return hit


_F8_CODE = {torch.float8_e4m3fn: 0, torch.float8_e5m2: 1}


def hip_fq8_linear_or_none(x8, layers):
    """y[.., sum N] = x . [fq(W_0); fq(W_1); ...]^T + bias through qt_linear_fq8_bf16: x8 holds the FP8 codes of the already
    fake-quantized activation, the bf16 weights of `layers` (QAT Linears that share it, stateless FP8 weight fake-quantizers
    of one format) are converted inside the kernel.  None when the kernel does not take the problem."""
    K = x8.shape[-1]
    if x8.dtype not in _F8_CODE or K % 128 != 0 or not x8.is_contiguous() or x8.data_ptr() % 16 or not 1 <= len(layers) <= 4:
        return None
    wf = layers[0].weight_fake_quant._qt_format
    for l in layers:
        W, f = l.weight, l.weight_fake_quant._qt_format
        if (W.dtype != torch.bfloat16 or not W.is_contiguous() or W.shape[1] != K or W.shape[0] % 16 or W.data_ptr() % 16
                or W.device != x8.device or f.key() != wf.key()):
            return None
        if l.bias is not None and (l.bias.dtype != torch.bfloat16 or not l.bias.is_contiguous() or l.bias.data_ptr() % 8
                                   or l.bias.device != x8.device):
            return None
    n = len(layers)
    M = x8.numel() // K
    ns = [l.weight.shape[0] for l in layers]
    y = torch.empty((M, sum(ns)), dtype=torch.bfloat16, device=x8.device)
    wp = (ctypes.c_void_p * n)(*[l.weight.data_ptr() for l in layers])
    bp = (ctypes.c_void_p * n)(*[(l.bias.data_ptr() if l.bias is not None else None) for l in layers])
    nn = (ctypes.c_int * n)(*ns)
    rc = _native.lib().qt_linear_fq8_bf16(x8.data_ptr(), _F8_CODE[x8.dtype], wp, bp, nn, n, 1 if wf.p0 == 2 else 0, y.data_ptr(),
                                           M, K, _stream_ptr(x8))
    if _native.declined(rc, dtype=True):
        return None
    _native.check(rc, "qt_linear_fq8_bf16")
    return y


def mark_fp8_producer(consumer, act_fq):
    """Called when the activation fake-quantizer of `consumer` is created: if `consumer` is a QAT Linear
    whose weight fake-quantizer and this activation fake-quantizer both produce exact FP8 values with
    scale 1 (e4m3 / e5m2 specs without `qs`), the activation pass also emits FP8 bytes for the GEMM."""
    from .modules.qat.linear import Linear as QATLinear
    if not (fp8_gemm_enabled() and isinstance(consumer, QATLinear)):
        return
    wfq = consumer.weight_fake_quant
    if isinstance(wfq, FusedAmaxObsFakeQuantize) and isinstance(act_fq, FusedAmaxObsFakeQuantize) \
            and wfq.fp8_exact() and act_fq.fp8_exact():
        act_fq._emit_fp8 = "both"


_WEIGHT_CACHE = {"on": False, "epoch": 0}      # harness.cache_quantized_weights(True) turns it on


def cache_quantized_weights(enable: bool = True):
    """Opt-in: in eval mode, with the weight fake-quantizer's observer off (stateless spec or frozen
    after calibration), fq(W) is a constant -- keep it instead of re-quantizing W on every forward.  Off by default
    because the reference re-quantizes every time (and the headline metric counts those elements).  Entries follow
    the tensors' version counters (optimizer steps, load_state_dict, in-place ops); a write through `.data` is not
    visible to them -- call this function again to drop every entry."""
    _WEIGHT_CACHE["on"] = bool(enable)
    _WEIGHT_CACHE["epoch"] += 1


def cached_weight(layer, kind, make):
    """make() -> quantized weight; cached on the layer while nothing it depends on changes."""
    fq = layer.weight_fake_quant
    W = layer.weight
    if (not _WEIGHT_CACHE["on"] or layer.training or getattr(fq, "_observe", True)
            or (torch.is_grad_enabled() and W.requires_grad)):
        return make()
    key = (kind, _WEIGHT_CACHE["epoch"], W.data_ptr(), W._version, fq.scale._version, bool(getattr(fq, "_quantize", True)),
           str(W.device))
    hit = layer.__dict__.get("_qt_wcache")
    if hit is not None and hit[0] == key:
        return hit[1]
    w = make()
    layer.__dict__["_qt_wcache"] = (key, w)
    return w


class SiblingGroup:
    """Linears that read the same tensor (q / k / v projections behind one RMSNorm).  When the first of them runs,
    every member's weight is fake-quantized to FP8 in one launch (qt_fake_quant_bf16_fp8_multi) into one [sum N, K]
    buffer and ONE FP8 GEMM multiplies the shared activation by all of them; the other members then return their
    column slice of that product.  Work per call is what the reference issues (each weight pass, each member's own
    input pass), only batched: three 22 us GEMMs + three 12.5 us weight passes become one 43 us GEMM + one 29 us pass.

    A member takes its slice only if its input is the fake-quantized image of the very tensor the leader saw
    (`_qt_origin` of the hook's output) and all members quantize inputs and weights with the same stateless FP8
    format, so the leader's FP8 activation IS theirs, byte for byte."""

    def __init__(self, layers, value_map_only=False):
        self.layers = list(layers)
        self.value_map_only = value_map_only   # gate / up: one launch only on the value-map GEMM (qt_linear_fqt_ws_bf16), see model_fusions
        self.buf = None
        self.bias = None                       # (key of the members' bias versions, concatenated bias [sum N])
        self.stash = None                      # (origin key, product [M, sum N], taken flags)

    def eligible(self):
        K = self.layers[0].weight.shape[1]
        w_fmt = a_fmt = None
        with_bias = self.layers[0].bias is not None
        for l in self.layers:
            W, fq = l.weight, l.weight_fake_quant
            if (l.bias is not None) != with_bias or (with_bias and (l.bias.dtype != torch.bfloat16 or l.bias.device != W.device)):
                return False
            if not (isinstance(fq, FusedAmaxObsFakeQuantize) and fq.fp8_exact() and W.dtype == torch.bfloat16
                    and W.is_contiguous() and W.shape[1] == K and K % 16 == 0 and W.shape[0] % 16 == 0
                    and not (torch.is_grad_enabled() and W.requires_grad)):
                return False
            holder = getattr(l, "activation_pre_process", None)
            afq = holder["0"] if holder is not None and "0" in holder else None
            if not (isinstance(afq, FusedAmaxObsFakeQuantize) and afq.producer_fusable()):
                return False
            if w_fmt is None:
                w_fmt, a_fmt = fq._qt_format.key(), afq._qt_format.key()
            elif fq._qt_format.key() != w_fmt or afq._qt_format.key() != a_fmt:
                return False
        return True

    def bias_or_none(self):
        """The members' biases as one [sum N] vector (BERT-style projections), rebuilt when any of them changes."""
        if self.layers[0].bias is None:
            return None
        key = tuple((l.bias.data_ptr(), l.bias._version) for l in self.layers)
        if self.bias is None or self.bias[0] != key:
            if torch.cuda.is_current_stream_capturing():
                return False                   # no allocation that outlives the graph from inside a capture
            self.bias = (key, torch.cat([l.bias.detach() for l in self.layers]))
        return self.bias[1]


def _origin_key(x):
    # a hook's output names its origin (unchecked read, as ever: it goes straight to its Linear); the leader's input was handed through by its hook
    return handover.origin(x, unchecked=True) or handover.tensor_key(x)


def hip_mlp_fq8_or_none(x8, gate, up, out_fq, codes_only=False):
    """(h, h8) = the gated MLP's front half in one launch (qt_mlp_fq8_bf16): fq_out(silu(gate(x)) * up(x)) as bf16 values and FP8
    codes from the FP8 codes of x and the UNQUANTIZED bf16 weights of the QAT Linears `gate` / `up`.  None when the kernel does
    not take the problem."""
    K = x8.shape[-1]
    Wg, Wu = gate.weight, up.weight
    fg, fu = gate.weight_fake_quant._qt_format, up.weight_fake_quant._qt_format
    if (x8.dtype not in _F8_CODE or K % 128 != 0 or not x8.is_contiguous() or x8.data_ptr() % 16 or Wg.shape != Wu.shape or fg.key() != fu.key()
            or Wg.shape[1] != K or Wg.shape[0] % 16):
        return None
    for W in (Wg, Wu):
        if W.dtype != torch.bfloat16 or not W.is_contiguous() or W.data_ptr() % 16 or W.device != x8.device:
            return None
    for l in (gate, up):
        if l.bias is not None and (l.bias.dtype != torch.bfloat16 or not l.bias.is_contiguous() or l.bias.data_ptr() % 8 or l.bias.device != x8.device):
            return None
    N = Wg.shape[0]
    M = x8.numel() // K
    h = torch.empty((M, N), dtype=torch.bfloat16, device=x8.device)
    h8 = torch.empty((M, N), dtype=torch.uint8, device=x8.device)
    rc = _native.lib().qt_mlp_fq8_bf16(x8.data_ptr(), _F8_CODE[x8.dtype], Wg.data_ptr(), Wu.data_ptr(),
                                        gate.bias.data_ptr() if gate.bias is not None else None, up.bias.data_ptr() if up.bias is not None else None,
                                        N, 1 if fg.p0 == 2 else 0, None if codes_only else h.data_ptr(), h8.data_ptr(),
                                        ctypes.byref(out_fq._qt_format), M, K, _stream_ptr(x8))      # codes_only: h stays unwritten (`_qt_lazy`)
    if _native.declined(rc, dtype=True):
        return None
    _native.check(rc, "qt_mlp_fq8_bf16")
    return h, h8


_MLP_CHOICE = {}          # (M, N, K, activation dtype, formats, device) -> True: one launch, False: two fused GEMMs + SiLU * up


# (M, N, K) -> the gated MLP's front half as ONE launch (qt_mlp_fq8_bf16) beats two fused GEMMs + SiLU * up; measured on MI355X
# (profiles/r02_mlp_fq8.txt and the window profiles: 114 us inside the LLaMA-2-7B window against 132 us for the three launches)
_MLP_TABLE = {
    (1024, 11008, 4096): True,
    (512, 11008, 4096): True,     # 67.3 / 96.5
}


def mlp_route_is_one_launch(x8, gate, up, out_fq):
    """Whether qt_mlp_fq8_bf16 runs the gated MLP's front half on this problem: QT_FQ8_MLP=2 forces it; else the committed table;
    else one launch where it fills the chip in a single round (a rule, never a measurement: see fq8_route_is_fused)."""
    if switches.mode("QT_FQ8_MLP") == "2":              # always (tests, ablations)
        return True
    K = x8.shape[-1]
    M = x8.numel() // K
    N = gate.weight.shape[0]
    hit = _MLP_TABLE.get((M, N, K))
    if hit is None:
        key = (M, N, K, x8.dtype, gate.weight_fake_quant._qt_format.key(), out_fq._qt_format.key(), x8.device.index)
        hit = _MLP_CHOICE.get(key)
        if hit is None:
            cus = torch.cuda.get_device_properties(x8.device).multi_processor_count
            hit = _MLP_CHOICE[key] = ((M + 255) // 256) * ((N // 16 + 5) // 6) <= cus
    _note_route("mlp", M, [N, N], K, "one_launch_gate_up_silu" if hit else "two_gemms+silu_mul")
    return hit


# ---- every FP8 weight pass of an evaluation forward as ONE launch (harness.GraphedBatch / GraphedWindow) -------------------------
# The weight-pass + library-GEMM route issues one codes-only pass per Linear (or per q / k / v group): 36 launches of ~5 us for a
# BERT-base batch.  The weights are constants of a forward and these fake-quantizers are stateless, so a captured forward may run
# all of them first, as one launch (qt_fake_quant_multi_bf16_fp8); each call site then finds its codes (precomputed.WEIGHT_CODES, a record
# on the Linear or its SiblingGroup: valid for the very next use, for those very tensors at those very versions) and counts its elements as before.
_W8_LOG = None            # while a warm-up forward is being recorded: [(owner, layers)] in call order


def start_weight_pass_log():
    global _W8_LOG
    _W8_LOG = []


def stop_weight_pass_log():
    global _W8_LOG
    log, _W8_LOG = _W8_LOG, None
    return log or []


def _note_weight_pass(owner, layers):
    if _W8_LOG is not None and all(o is not owner for o, _ in _W8_LOG):
        _W8_LOG.append((owner, tuple(layers)))


def _take_weight_codes(owner, layers):
    """What BatchedWeightCodes.launch() left for this forward of `owner` (precomputed.WEIGHT_CODES), if its weights are still those."""
    if precomputed.WEIGHT_CODES.name not in owner.__dict__:
        return None
    codes = precomputed.WEIGHT_CODES.take(owner, [l.weight for l in layers])
    return None if codes is precomputed.MISS else codes


# one launch of BatchedWeightCodes: the [(owner, layers, codes buffer)] of one weight format and the device item table (`count` rows)
_CodesLaunch = collections.namedtuple("_CodesLaunch", "fmt members items count tiles")


class BatchedWeightCodes:
    """`entries`: [(owner, layers)] as logged by a warm-up forward -- owner is the QAT Linear itself or its SiblingGroup (whose members'
    codes are one [sum N, K] buffer).  One launch per weight format."""

    def __init__(self, entries, device):
        self.groups = {}
        for owner, layers in entries:
            fq = layers[0].weight_fake_quant
            if not all(l.weight.device == device and l.weight.dtype == torch.bfloat16 and l.weight.is_contiguous() and l.weight.numel() % 16 == 0
                       and l.weight.data_ptr() % 16 == 0 and l.weight_fake_quant._qt_format.key() == fq._qt_format.key() for l in layers):
                continue
            fq._move_to(device)
            K = layers[0].weight.shape[1]
            total = sum(l.weight.shape[0] for l in layers)
            codes = torch.empty((total, K), dtype=torch.uint8, device=device)
            fmt, members = self.groups.setdefault(fq._qt_format.key(), (fq._qt_format, []))
            members.append((owner, layers, codes))
        self.launches = []
        for fmt, members in self.groups.values():
            rows, tiles = [], 0
            for owner, layers, codes in members:
                off = 0
                for l in layers:
                    npair = l.weight.numel() // 16
                    rows.append([l.weight.data_ptr(), codes.data_ptr() + off, npair, tiles])
                    tiles += (npair + 1023) // 1024
                    off += l.weight.numel()
            self.launches.append(_CodesLaunch(fmt, members, torch.tensor(rows, dtype=torch.int64, device=device), len(rows), tiles))

    def __len__(self):
        return sum(len(b.members) for b in self.launches)

    def launch(self):
        for b in self.launches:
            _native.check(_native.lib().qt_fake_quant_multi_bf16_fp8(b.items.data_ptr(), b.count, b.tiles, ctypes.byref(b.fmt), _stream_ptr(b.items)),
                          "qt_fake_quant_multi_bf16_fp8")
            for owner, layers, codes in b.members:
                precomputed.WEIGHT_CODES.leave(owner, [l.weight for l in layers], handover.fp8_view(codes, b.fmt))

    def forget(self):
        for b in self.launches:
            for owner, _, _ in b.members:
                precomputed.WEIGHT_CODES.drop(owner)


def _sibling_linear_or_none(layer, x, x8):
    group = layer.__dict__.get("_qt_sibling_group")
    if group is None or group.value_map_only or not switches.on("QT_SIBLING_GEMM") or _WEIGHT_CACHE["on"]:
        return None
    idx = group.layers.index(layer)
    key = _origin_key(x)
    Ns = [l.weight.shape[0] for l in group.layers]
    off = sum(Ns[:idx])
    if idx > 0:
        st = group.stash
        if st is None or st[0] != key or st[2][idx]:
            return None                        # not the leader's tensor (or already taken): the ordinary single path
        st[2][idx] = True
        STATS.add(layer.weight.numel())        # this member's weight pass ran inside the batched launch
        return st[1][:, off:off + Ns[idx]].reshape(*x.shape[:-1], Ns[idx])
    group.stash = None
    if not group.eligible():
        return None
    K = layer.weight.shape[1]
    total = sum(Ns)
    dev = x.device
    n = len(group.layers)
    if fq8_gemm_enabled() and fq8_route_is_fused(x8.reshape(-1, K), group.layers):
        layer.weight_fake_quant._move_to(dev)
        y = hip_fq8_linear_or_none(x8.reshape(-1, K), group.layers)
        if y is not None:
            STATS.add(layer.weight.numel())
            group.stash = (key, y, [True] + [False] * (n - 1))
            return y[:, :Ns[0]].reshape(*x.shape[:-1], Ns[0])
    fq = layer.weight_fake_quant
    fq._move_to(dev)
    w8 = _take_weight_codes(group, group.layers)              # BatchedWeightCodes ran this group's pass in front of the forward
    if w8 is None:
        if group.buf is None or group.buf.device != dev or group.buf.shape != (total, K):
            if torch.cuda.is_current_stream_capturing():
                return None
            group.buf = torch.empty((total, K), dtype=torch.uint8, device=dev)
        L = _native.lib()
        xs = (ctypes.c_void_p * n)(*[l.weight.data_ptr() for l in group.layers])
        ns = (ctypes.c_size_t * n)(*[l.weight.numel() for l in group.layers])
        _native.check(L.qt_fake_quant_bf16_fp8_multi(xs, ns, n, group.buf.data_ptr(), ctypes.byref(fq._qt_format),
                                                     _stream_ptr(x)), "qt_fake_quant_bf16_fp8_multi")
        w8 = handover.fp8_view(group.buf, fq)
        _note_weight_pass(group, group.layers)
    bias = group.bias_or_none()
    if bias is False:
        return None
    y = lt_fp8_gemm(x8.reshape(-1, K), w8, bias)
    if y is None:
        return None                            # library route unavailable: every member takes the ordinary path
    STATS.add(layer.weight.numel())
    group.stash = (key, y, [True] + [False] * (n - 1))
    return y[:, :Ns[0]].reshape(*x.shape[:-1], Ns[0])


def fp8_linear_or_none(layer, x):
    """E4M3 / E5M2 fake-quant Linear with scale 1 on the FP8 matrix cores: the activation pass already
    produced FP8 bytes (handover.codes(x)), the weight pass writes FP8 only (3 B/element of traffic instead of
    4 and nothing for the GEMM to re-read in bf16), and the products q_x * q_w are exactly the
    reference's bf16 products; fp32 accumulation, bf16 output.  Library FP8 GEMM (hipBLASLt through
    torch._scaled_mm) -- a plain GEMM on already-quantized operands."""
    x8 = handover.codes(x)
    fq = layer.weight_fake_quant
    if x8 is None or not fp8_gemm_enabled() or not isinstance(fq, FusedAmaxObsFakeQuantize) or not fq.fp8_exact():
        return None
    if torch.is_grad_enabled() and (layer.weight.requires_grad or x.requires_grad):
        return None
    W = layer.weight
    K = W.shape[1]
    if W.dtype != torch.bfloat16 or not W.is_contiguous() or K % 16 != 0 or W.shape[0] % 16 != 0:
        return None
    if layer.bias is not None and layer.bias.dtype != torch.bfloat16:
        return None
    fq._move_to(x.device)
    shared = _sibling_linear_or_none(layer, x, x8)
    if shared is not None:
        return shared
    if fq8_gemm_enabled() and not _WEIGHT_CACHE["on"] and fq8_route_is_fused(x8.reshape(-1, K), [layer]):
        y = hip_fq8_linear_or_none(x8.reshape(-1, K), [layer])
        if y is not None:
            STATS.add(W.numel())                   # the weight's fake-quant call, computed inside the GEMM
            return y.reshape(*x.shape[:-1], W.shape[0])
    def make():
        STATS.add(W.numel())
        return FusedAmaxObsFakeQuantFunction.apply(W.detach(), False, True, fq.qmap, fq.amax_history, fq.scale,
                                                   fq.amax_history_len, fq.quant_max, None, False, False,
                                                   fq._qt_format, "only")
    w8 = _take_weight_codes(layer, (layer,))                   # BatchedWeightCodes ran this pass in front of the forward
    if w8 is not None:
        STATS.add(W.numel())
    else:
        w8 = cached_weight(layer, "fp8", make)
        if not _WEIGHT_CACHE["on"]:
            _note_weight_pass(layer, (layer,))
    one = _one(x.device)
    x2 = x8.reshape(-1, K)
    y = lt_fp8_gemm(x2, w8, layer.bias)
    if y is None:
        y = torch._scaled_mm(x2, w8.t(), scale_a=one, scale_b=one, bias=layer.bias, out_dtype=torch.bfloat16)
    return y.reshape(*x.shape[:-1], W.shape[0])


_LT = {"ok": True, "ws": {}}                  # "ok" turns False when libhipblaslt cannot be resolved in the process

# Which of hipBLASLt's suggestions runs a problem: (batch, M, N, K, b_is_kn, bias) -> index into the library's ordered list.
# Measured once on MI355X by tools/tune_lt_algos.py (profiles/r05_lt_algos.txt: microseconds of every suggestion) and COMMITTED, so
# every process, rank and box runs the same library kernel -- the same order of fp32 additions -- for a shape; rounds 1-4 timed the
# suggestions in each process and two ranks could disagree.  Shapes not listed run the library's first suggestion (index 0).
_LT_ALGO_TABLE = {
    (1, 6144, 768, 3072, 0, 1): 3,        # BERT-base output dense: 20.2 us against 22.1 for the first suggestion
    (1, 2048, 4096, 4096, 0, 0): 1,       # 32.2 / 35.5
    (1, 1024, 5120, 13824, 0, 0): 5,      # 71.1 / 80.0
    (1, 1024, 5120, 5120, 0, 0): 2,       # 31.8 / 33.4
    (40, 1024, 1024, 128, 0, 0): 1,       # 13B Q.K^T chain: 26.9 / 27.8
    (40, 1024, 128, 1024, 1, 0): 2,       # 13B P.V chain: 19.8 / 31.6
    (192, 384, 384, 64, 0, 0): 12,        # BERT-base Q.K^T chain: 56.3 / 66.6
    (192, 384, 64, 384, 1, 0): 5,         # BERT-base P.V chain: 13.5 / 32.6
}
# The positions above are positions in the suggestion list of ONE build of the library (hipblasLtGetVersion; ROCm 7.2.0: hipblasLtGetVersion = 100000;
# 1.2.1).  Under any other build the same index would silently name another kernel, so the table is ignored there: every shape runs the
# library's first suggestion and routes_report() says so ("lt:library_version").
_LT_ALGO_TABLE_LIBRARY = 100000
LT_ALGOS = {}              # what ran: "bxMxNxK[kn][+bias]" -> index (routes_report)
_LT_LIBRARY = {"version": None}


def lt_table_applies():
    """True when the resolved hipBLASLt is the build _LT_ALGO_TABLE was measured on (or does not report a version at all)."""
    if _LT_LIBRARY["version"] is None:
        _LT_LIBRARY["version"] = int(_native.lib().qt_fp8_gemm_library_version())
        if _LT_LIBRARY["version"] not in (0, _LT_ALGO_TABLE_LIBRARY):
            LT_ALGOS["lt:library_version"] = f"{_LT_LIBRARY['version']} != table's {_LT_ALGO_TABLE_LIBRARY}: first suggestion everywhere"
    return _LT_LIBRARY["version"] in (0, _LT_ALGO_TABLE_LIBRARY)


def lt_algo_index(batch, M, N, K, b_is_kn, with_bias):
    forced = switches.raw("QT_LT_ALGO")                     # tools only: the tuner's A/B runs
    idx = int(forced) if forced is not None else _LT_ALGO_TABLE.get((batch, M, N, K, int(bool(b_is_kn)), int(bool(with_bias))), 0)
    if forced is None and idx and not lt_table_applies():
        idx = 0
    LT_ALGOS.setdefault(f"lt:{batch}x{M}x{N}x{K}{'kn' if b_is_kn else ''}{'+bias' if with_bias else ''}", idx)
    return idx


def lt_fp8_gemm(a8, b8, bias=None, b_is_kn=False):
    """C = A . op(B) on FP8 operands through qt_fp8_gemm (hipBLASLt; which of its suggestions runs is a committed table, _LT_ALGO_TABLE).  a8 [.., M, K];
    b8 [N, K] (b_is_kn False) or [.., K, N] (True); leading dims of a8 / b8 are a batch.  None when the library route is
    unavailable for this problem (the caller falls back to torch._scaled_mm / bf16)."""
    if not _LT["ok"] or not switches.on("QT_LT_GEMM"):
        return None
    dev = a8.device
    ws = _LT["ws"].get(dev)
    if ws is None:
        ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
        _LT["ws"][dev] = ws
    fmt = {torch.float8_e4m3fn: 0, torch.float8_e5m2: 1}
    if a8.dtype not in fmt or b8.dtype not in fmt or not a8.is_contiguous() or not b8.is_contiguous():
        return None
    M, K = a8.shape[-2], a8.shape[-1]
    if b_is_kn:
        N = b8.shape[-1]
        if b8.shape[-2] != K or b8.shape[:-2] != a8.shape[:-2]:
            return None
    else:
        N = b8.shape[-2]
        if b8.shape[-1] != K or (b8.dim() > 2 and b8.shape[:-2] != a8.shape[:-2]):
            return None
    batch = 1
    for d in a8.shape[:-2]:
        batch *= d
    b_stride = 0 if b8.dim() == 2 else N * K
    out = torch.empty(a8.shape[:-1] + (N,), dtype=torch.bfloat16, device=dev)
    rc = _native.lib().qt_fp8_gemm(a8.data_ptr(), fmt[a8.dtype], b8.data_ptr(), fmt[b8.dtype], int(b_is_kn), out.data_ptr(),
                                   bias.data_ptr() if bias is not None else None, batch, M, N, K, M * K, b_stride, M * N,
                                   ws.data_ptr(), ws.numel(), lt_algo_index(batch, M, N, K, b_is_kn, bias is not None), _stream_ptr(a8))
    if rc != 0:
        if rc in (_native.QT_ERR_NO_DEVICE,):
            _LT["ok"] = False                      # the library cannot be resolved in this process: stop trying
        return None
    return out


_ONES = {}


def _one(device):
    t = _ONES.get(device)
    if t is None:
        t = torch.ones((), dtype=torch.float32, device=device)
        _ONES[device] = t
    return t


def _operand(fq, device):
    """qt_operand_q for a weight fake-quantizer (per-tensor only)."""
    op = _native.QtOperandQ()
    op.fmt = fq._qt_format
    op.lut_dev = fq.qmap.data_ptr() if fq._qt_format.kind == _native.QT_FMT_LUT else None
    op.scale_f32_dev = None if fq.qscheme is None and getattr(fq, "_scale_is_one", True) else fq.scale.data_ptr()
    op.amax_bits_dev = fq.amax_history.data_ptr() if fq._observe else None
    return op


def fused_linear_or_none(layer, x):
    """y = x @ fq(W)^T + b with W fake-quantized while its tiles are staged (qt_linear_fq_bf16).
    Applies to bf16 device tensors under no_grad with a per-tensor weight fake-quantizer."""
    out = fp8_linear_or_none(layer, x)
    if out is not None:
        return out
    handover.materialize(x)                      # every other route reads the values: a producer may have written the FP8 codes only
    out = fqt_linear_or_none(layer, x)
    if out is not None:
        return out
    fq = layer.weight_fake_quant
    W = layer.weight
    if not (fused_gemm_enabled() and isinstance(fq, FusedAmaxObsFakeQuantize)):
        return None
    if torch.is_grad_enabled() and (W.requires_grad or x.requires_grad):
        return None
    if not (x.device.type == "cuda" and x.dtype == torch.bfloat16 and W.dtype == torch.bfloat16):
        return None
    if fq.is_per_channel or fq.qscheme in (QScheme.MICROSCALING, QScheme.GROUP_WISE_AFFINE):
        return None
    if fq.outlier_threshold is not None or fq.record_histogram or not fq._quantize:
        return None
    if fq._qt_format.kind == _native.QT_FMT_LUT:
        return None       # table formats: elementwise pass (LDS-staged table) + library GEMM is faster
    K = W.shape[1]
    if K % 8 != 0 or not W.is_contiguous() or (layer.bias is not None and layer.bias.dtype != torch.bfloat16):
        return None
    L = _native.lib()
    fq._move_to(x.device)
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M, N = x2.shape[0], W.shape[0]
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    st = _stream_ptr(x)
    if fq._observe:
        if fq.amax_history.numel() == 0:
            fq.amax_history.resize_((fq.amax_history_len,)).fill_(0.0)
            fq.scale.resize_(()).fill_(1.0)
        launch_scale_update(fq.amax_history, fq.scale, fq.quant_max, fq.force_scale_power_of_two, st)
    qw = _operand(fq, x.device)
    qx = _native.QtOperandQ()
    qx.fmt = _IDENTITY
    code = L.qt_linear_fq_bf16(x2.data_ptr(), W.data_ptr(),
                               layer.bias.data_ptr() if layer.bias is not None else None,
                               y.data_ptr(), M, N, K, ctypes.byref(qx), ctypes.byref(qw), st)
    _native.check(code, "qt_linear_fq_bf16")
    STATS.add(W.numel())
    return y.reshape(*x.shape[:-1], N)


# ---- any stateless value map on the weight: bf16 GEMM with the map applied in its operand path (qt_linear_fqt_bf16) --------
_FQT_TABLES = {}          # (dtype, device) -> dict: rows / map device tensors, signed_rows, sign_mask, usable


def fqt_gemm_mode():
    """QT_FQT_GEMM: "auto" (default) -- the fused kernel for the problem shapes where it measured faster than the weight pass +
    library GEMM pair (a fixed rule, `fqt_route_is_fused`: no timing at run time, every rank and every run takes the same route);
    "1" -- wherever the kernel takes the problem; "0" -- never."""
    return switches.mode("QT_FQT_GEMM")


def fqt_tables(fq, device):
    """Row form of `fq`'s value map on `device` (built once per dtype and device): None when the map has flagged rows inside
    the range weights live in (2^-40 .. 2^15), where the kernel would keep falling back to its slow path."""
    key = (str(fq.dtype), str(device))
    hit = _FQT_TABLES.get(key)
    if hit is None:
        import numpy as np
        m = _native.build_map_u16(fq.dtype)
        rp = _native.build_rowparams(m)
        rows = np.ctypeslib.as_array(rp.row).reshape(2048).astype(np.uint32)
        flagged = np.ctypeslib.as_array(rp.flagged)
        lo, hi = 127 - 40, 127 + 15
        usable = not flagged[lo:hi].any() and not (rp.signed_rows and flagged[256 + lo:256 + hi].any())
        hit = {"rows": torch.from_numpy(rows.view(np.int32).copy()).to(device), "map": torch.from_numpy(m.view(np.int16).copy()).to(device),
               "signed": int(rp.signed_rows), "mask": int(rp.sign_mask), "usable": bool(usable)}
        _FQT_TABLES[key] = hit
    return hit if hit["usable"] else None


def fqt_plan(M, n_total, K):
    """(ksplit, workspace bytes, tickets) qt_linear_fqt_ws_bf16 would use for this problem (host-only query)."""
    ks, wb, nt = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    _native.check(_native.lib().qt_linear_fqt_plan(M, n_total, K, ctypes.byref(ks), ctypes.byref(wb), ctypes.byref(nt)), "qt_linear_fqt_plan")
    return ks.value, wb.value, nt.value


def fqt_route_is_fused(M, ns, K, device):
    """Fixed routing rule for qt_linear_fqt_ws_bf16, from same-box A/B runs of the whole configs[3] window (tools/ab_13b_routes.py,
    profiles/r04_13b_route_ab.txt; MI355X, posit(8,2)): the kernel takes every Linear whose 512-row tiles are at least five column
    groups wide on a full chip -- q / k / v as one launch, the lm head, and since round 4 gate / up too: alone it ties with the weight
    pass + library GEMM (161-183 against 173-179 us), inside the window it is worth 2.4 ms of 37 (the pair's pass and GEMM compete
    with their neighbours for HBM) -- and, with split-K, narrow outputs with a deep K (down: 1024 x 5120 x 13824, three workgroups
    per 512 x 128 tile, 144 k steps each: 167-177 against 181-200 us).  It loses where a split's k range is too short to pay for
    the hand-off of the fp32 partial sums (o: 1024 x 5120 x 5120, 83 against 70 us; +0.2 ms per window), which stays on the pair."""
    mode = fqt_gemm_mode()
    if mode != "auto":
        return mode == "1"
    if M <= 256 or K % 32:
        return False
    ksplit = fqt_plan(M, sum(ns), K)[0]
    if ksplit > 1:
        return (K // 32) // ksplit >= 128
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    groups = sum(ns) // 16
    tiles_m = (M + 511) // 512
    tn_min = (groups + 7) // 8
    rounds = (tiles_m * tn_min + cus - 1) // cus
    tn = max(tn_min, rounds * cus // tiles_m)
    return groups / tn >= 5.0 and tiles_m * tn >= 0.9 * rounds * cus


def _fqt_route(M, ns, K, device):
    hit = fqt_route_is_fused(M, ns, K, device)
    _note_route("fqt", M, ns, K, "fused_value_map_gemm" if hit else "weight_pass+library_bf16_gemm")
    return hit


def hip_fqt_linear_or_none(x2, layers, tables):
    """y[M, sum N] = x2 . [fq(W_0); fq(W_1); ...]^T + bias through qt_linear_fqt_bf16: x2 [M, K] holds the bf16 VALUES of the already
    fake-quantized activation, the bf16 weights of `layers` go through the row form of their value map inside the kernel."""
    M, K = x2.shape
    if x2.dtype != torch.bfloat16 or K % 32 or not x2.is_contiguous() or x2.data_ptr() % 16 or not 1 <= len(layers) <= 4:
        return None
    for l in layers:
        W = l.weight
        if (W.dtype != torch.bfloat16 or not W.is_contiguous() or W.shape[1] != K or W.shape[0] % 16 or W.data_ptr() % 16 or W.device != x2.device):
            return None
        if l.bias is not None and (l.bias.dtype != torch.bfloat16 or not l.bias.is_contiguous() or l.bias.data_ptr() % 8 or l.bias.device != x2.device):
            return None
    n = len(layers)
    ns = [l.weight.shape[0] for l in layers]
    y = torch.empty((M, sum(ns)), dtype=torch.bfloat16, device=x2.device)
    wp = (ctypes.c_void_p * n)(*[l.weight.data_ptr() for l in layers])
    bp = (ctypes.c_void_p * n)(*[(l.bias.data_ptr() if l.bias is not None else None) for l in layers])
    nn = (ctypes.c_int * n)(*ns)
    _native.note_device(x2.device.index)
    ws, tickets = _fqt_workspace(M, sum(ns), K, x2.device)
    rc = _native.lib().qt_linear_fqt_ws_bf16(x2.data_ptr(), wp, bp, nn, n, tables["rows"].data_ptr(), tables["signed"], tables["mask"],
                                              tables["map"].data_ptr(), y.data_ptr(), M, K,
                                              ws.data_ptr() if ws is not None else None, ws.numel() * 4 if ws is not None else 0,
                                              tickets.data_ptr() if tickets is not None else None, tickets.numel() if tickets is not None else 0,
                                              _stream_ptr(x2))
    if _native.declined(rc, dtype=True):
        return None
    _native.check(rc, "qt_linear_fqt_ws_bf16")
    return y


# Split-K scratch (qt_linear_fqt_ws_bf16): an fp32 workspace and a ticket array that ONE ordered sequence of
# launches may share -- so they are keyed by (kernel, device, stream, capture): every eager stream and every captured graph has its
# own (include/qt_hip.h: "launches that share a workspace must be ordered on one stream"; a graph replay may overlap eager work on
# another stream, and a second capture may be replayed beside the first).  Inside a capture the buffers come from the graph's
# memory pool (the zero fill of the tickets becomes a node of the graph; every launch leaves them zero anyway).  Outgrown buffers
# stay allocated: a hipGraph captured earlier replays launches that hold their addresses.
_SPLITK_WS = {}
_SPLITK_WS_OLD = []


def _capture_id(stream_ptr):
    cid = ctypes.c_ulonglong(0)
    _native.check(_native.lib().qt_stream_capture_id(stream_ptr, ctypes.byref(cid)), "qt_stream_capture_id")
    return cid.value


def splitk_scratch(kind, wbytes, ntick, device):
    """(workspace, tickets) for the launch about to be issued on `device`'s current stream."""
    st = torch.cuda.current_stream(device).cuda_stream
    key = (kind, device.index if device.index is not None else torch.cuda.current_device(), st, _capture_id(ctypes.c_void_p(st)))
    ws, tickets = _SPLITK_WS.get(key, (None, None))
    if ws is None and len(_SPLITK_WS) > 8:
        # entries of captures that have ended: the graph's pool keeps their memory alive for its replays, this table need not
        for k in [k for k in _SPLITK_WS if k[3] not in (0, key[3])]:
            del _SPLITK_WS[k]
    if ws is None or ws.numel() * 4 < wbytes or tickets.numel() < ntick:
        if ws is not None:
            _SPLITK_WS_OLD.append((ws, tickets))
        ws = torch.empty(((wbytes + 3) // 4,), dtype=torch.float32, device=device)
        tickets = torch.zeros((max(ntick, 4096),), dtype=torch.int32, device=device)
        _SPLITK_WS[key] = (ws, tickets)
    return ws, tickets


def _fqt_workspace(M, n_total, K, device):
    ksplit, wbytes, ntick = fqt_plan(M, n_total, K)
    if ksplit <= 1:
        return None, None
    return splitk_scratch("fqt", wbytes, ntick, device)


def _fqt_weight_ok(layer):
    fq = layer.weight_fake_quant
    return (isinstance(fq, FusedAmaxObsFakeQuantize) and fq.stateless_map() and fq._qt_format.kind != _native.QT_FMT_IDENTITY
            and not fq.fp8_exact())


def fqt_linear_or_none(layer, x):
    """The fake-quant Linear of a stateless non-FP8 weight spec (posit, intN, fp6 / fp4 without `qs`) as ONE launch: the weight's
    value map is applied inside the bf16 GEMM, fq(W) is never written.  q / k / v projections that read the same fake-quantized
    tensor (same stateless input format) share a launch through their SiblingGroup.  None when the rule above prefers the weight
    pass + library GEMM, or the kernel does not take the problem."""
    if fqt_gemm_mode() == "0" or not _fqt_weight_ok(layer):
        return None
    W = layer.weight
    if torch.is_grad_enabled() and (W.requires_grad or x.requires_grad):
        return None
    if not (x.device.type == "cuda" and x.dtype == torch.bfloat16 and W.dtype == torch.bfloat16) or _WEIGHT_CACHE["on"]:
        return None
    K = W.shape[1]
    fq = layer.weight_fake_quant
    tables = fqt_tables(fq, x.device)
    if tables is None:
        return None
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    group = layer.__dict__.get("_qt_sibling_group")
    if group is not None and group.value_map_only and not switches.on("QT_GATE_UP_GROUP"):      # A/B hook (tools/ab_13b_routes.py)
        group = None
    if group is not None and switches.on("QT_SIBLING_GEMM"):
        idx = group.layers.index(layer)
        Ns = [l.weight.shape[0] for l in group.layers]
        key = _origin_key(x)
        if idx > 0:
            st = group.stash
            if st is not None and st[0] == ("fqt",) + tuple(key) and not st[2][idx]:
                st[2][idx] = True
                STATS.add(W.numel())
                off = sum(Ns[:idx])
                return st[1][:, off:off + Ns[idx]].reshape(*x.shape[:-1], Ns[idx])
        else:
            group.stash = None
            same = all(_fqt_weight_ok(l) and str(l.weight_fake_quant.dtype) == str(fq.dtype) and l.weight.shape[1] == K
                       and (l.bias is None) == (layer.bias is None) for l in group.layers)
            afq = [getattr(l, "activation_pre_process", None) for l in group.layers]
            afq = [h["0"] if h is not None and "0" in h else None for h in afq]
            same = same and all(isinstance(f, FusedAmaxObsFakeQuantize) and f.stateless_map() and str(f.dtype) == str(afq[0].dtype) for f in afq)
            # x is the fake-quantized image of one tensor: a hook's output (`_qt_origin`), or a producer kernel's result that the leader's
            # hook handed through (model_fusions.rmsnorm_map; the siblings' hooks then name it as their origin)
            shared = handover.origin(x, unchecked=True) is not None or handover.done_by(x) is not None      # (origin: unchecked, as in _origin_key)
            if same and shared and _fqt_route(M, Ns, K, x.device):
                if not x2.is_contiguous():
                    x2 = x2.contiguous()
                y = hip_fqt_linear_or_none(x2, group.layers, tables)
                if y is not None:
                    STATS.add(W.numel())
                    group.stash = (("fqt",) + tuple(key), y, [True] + [False] * (len(Ns) - 1))
                    return y[:, :Ns[0]].reshape(*x.shape[:-1], Ns[0])
    if not _fqt_route(M, [W.shape[0]], K, x.device):
        return None
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    y = hip_fqt_linear_or_none(x2, [layer], tables)
    if y is None:
        return None
    STATS.add(W.numel())
    return y.reshape(*x.shape[:-1], W.shape[0])
