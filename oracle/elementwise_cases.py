"""The inputs of the elementwise kernel tests (tests/test_gpu_elementwise_ops.py) -- TEST INFRASTRUCTURE ONLY, numpy only.

Deterministic, so that tests/test_oracle_elementwise_cpu.py (no GPU) and the GPU tests see the same tensors.  Three families:

  rotary     x [B, S, H, D] for q and k (Hk <= Hq) and a value tensor, N(0, 2); cos / sin [B, S, D] from real angles (position * theta^(-2j/D),
             HF's layout cat(f, f)).  Exact zeros every 1013th element (the flagged row 0 of posit maps).  Where they fit, all 65 536 bf16
             patterns as x (from token 2 on).  Token 1 carries the planted edges, in head 0 of q and of k (PLANTS below).
  SiLU * up  gates N(0, sigma), sigma cycling over 1, 3, 8 by row, ups N(0, 1): the well-conditioned regime.  Behind it (mask `well` False):
             the planted gates (SILU_GATES) against ups of every sign and class, ups that take the product into the FP8 saturation range,
             and, where they fit, all patterns as the gate and all patterns as the up.
  GELU       N(0, 1.5): the well-conditioned regime; planted values and, where they fit, all patterns behind it.
"""
import numpy as np

from . import qt_oracle as o
from .row_cases import _seed

U16 = np.uint16
ONE, MINUS_ONE, NEG_ZERO, MIN_NORMAL, SUBNORMAL, POS_INF, NEG_INF, NAN, MAX, NEG_MAX = (0x3F80, 0xBF80, 0x8000, 0x0080, 0x0001, 0x7F80, 0xFF80, 0x7FC0,
                                                                                      0x7F7F, 0xFF7F)
SMALL = 0x1F40              # 1.5 * 2^-65: the product of two of them is 2.25 * 2^-130, in the fp32 (and bf16) subnormal range
HALF = 0x3F00

# (d, x[d], x[d + D/2], cos[d], sin[d]) planted on token 1, head 0 (d < 8 <= D/2: the low half, y[d] = x[d] cos[d] - x[d + D/2] sin[d])
PLANTS = (
    (0, POS_INF, POS_INF, ONE, ONE),               # inf - inf = NaN
    (1, MAX, NEG_MAX, ONE, ONE),                   # max + max: the fp32 sum rounds to bf16 inf (NaN behind a consumer's fake-quantizer)
    (2, POS_INF, ONE, 0x0000, ONE),                # inf * 0 = NaN
    (3, SMALL, 0x0000, SMALL, 0x0000),             # an fp32-subnormal product that bf16 keeps (2.25 * 2^-130 -> 2^-129)
    (4, SUBNORMAL, SMALL, HALF, SMALL),            # 2^-134 + an fp32-subnormal product: both round away in bf16, in a fixed direction
    (5, 0x4040, 0x4768, NEG_ZERO, MINUS_ONE),      # 3 * -0 + 59392: finite, beyond both FP8 maxima -- the consumer saturates
    (6, 0x4040, 0x4000, NAN, ONE),                 # NaN in the table
    (7, MAX, ONE, MIN_NORMAL, SUBNORMAL),          # the smallest normal and a subnormal in the tables
)


def _bits(a):
    return o.f32_to_bf16(np.asarray(a, np.float32))


def _normal(rng, shape, sigma):
    return _bits(rng.standard_normal(shape, dtype=np.float32) * np.float32(sigma))


def rope_tables(B, S, D, theta=10000.0):
    """cos, sin [B, S, D] bf16 patterns: batch b starts at position 3 b."""
    pos = (np.arange(S)[None, :] + 3 * np.arange(B)[:, None]).astype(np.float64)
    inv = theta ** (-np.arange(0, D, 2, dtype=np.float64) / D)
    f = pos[..., None] * inv
    f = np.concatenate([f, f], axis=-1)
    return _bits(np.cos(f)), _bits(np.sin(f))


def rope_case(B, S, Hq, Hk, D, value=False, planted=True):
    """dict(q [B, S, Hq, D], k [B, S, Hk, D], cos, sin [B, S, D], v [B, S, Hk, D] or None, patterns: whether q holds every pattern)."""
    rng = np.random.default_rng(_seed("rope", B, S, Hq, Hk, D))
    cos, sin = rope_tables(B, S, D)
    out = {"cos": cos, "sin": sin, "v": None, "patterns": False}
    for name, H in (("q", Hq), ("k", Hk)) + ((("v", Hk),) if value else ()):
        x = _normal(rng, (B, S, H, D), 2.0)
        flat = x.reshape(-1)
        flat[::1013] = 0
        first = 2 * H * D                                          # (tokens 0 and 1 stay as they are)
        if flat.size >= first + 65536:
            flat[first:first + 65536] = o.all_bf16_patterns()
            if name == "q":
                out["patterns"] = True
        out[name] = x
    if planted and B * S >= 2 and D >= 16:
        b, s = divmod(1, S)
        for d, x0, x1, c, sn in PLANTS:
            cos[b, s, d], sin[b, s, d] = c, sn
            for name in ("q", "k"):
                out[name][b, s, 0, d], out[name][b, s, 0, d + D // 2] = x0, x1
        if value:                                                  # the value job sees the non-finite classes and the saturation range too
            out["v"][b, s, 0, :8] = (POS_INF, NEG_INF, NAN, MAX, NEG_MAX, NEG_ZERO, SUBNORMAL, 0x43E8)
    return out


def qkv_rows(c):
    """The case as column slices of ONE wider buffer, as the projections' GEMM leaves them: uint16 [B * S, rs] with q | k | v | 16 columns
    of NaN.  Returns (buffer, rs, column of q, of k, of v)."""
    B, S, Hq, D = c["q"].shape
    Hk = c["k"].shape[2]
    T = B * S
    parts = [c["q"].reshape(T, Hq * D), c["k"].reshape(T, Hk * D)] + ([c["v"].reshape(T, Hk * D)] if c["v"] is not None else [])
    buf = np.concatenate(parts + [np.full((T, 16), NAN, U16)], axis=1)
    return np.ascontiguousarray(buf), buf.shape[1], 0, Hq * D, (Hq + Hk) * D


def tokens_as(T):
    """(B, S) with B * S == T and B > 1 where T has a small factor."""
    for B in (3, 2, 5, 7):
        if T % B == 0 and T > B:
            return B, T // B
    return 1, T


# ---- SiLU * up --------------------------------------------------------------------------------------------------------------------------
SILU_GATES = (0xC2B1, 0xC2B2, 0x0000, NEG_ZERO, POS_INF, NEG_INF, NAN, MAX, NEG_MAX, 0xC2B0, 0xC300, SUBNORMAL)    # -88.5, -89, ..., -88, -128
SILU_UPS = (ONE, MINUS_ONE, 0x0000, POS_INF, NAN, MAX, 0x43E8, 0x4768)                                             # ..., 464, 59392
SILU_SIGMAS = (1.0, 3.0, 8.0)


def silu_case(rows, cols):
    """dict(gate, up [rows, cols] patterns, well: bool mask of the well-conditioned regime, patterns: whether all patterns are there).
    The planted part grows with the tensor: 8 elements at 1 x 8, every gate against every up from 96 elements on, the saturating ups
    from 1024 on, all patterns from 2^18 on."""
    rng = np.random.default_rng(_seed("silu", rows, cols))
    sig = np.asarray(SILU_SIGMAS, np.float32)[np.arange(rows) % 3][:, None]
    gate = _bits(rng.standard_normal((rows, cols), dtype=np.float32) * sig)
    up = _normal(rng, (rows, cols), 1.0)
    well = np.ones(rows * cols, bool)
    g, u = gate.reshape(-1), up.reshape(-1)
    n = g.size
    pairs = [(a, b) for b in SILU_UPS for a in SILU_GATES]
    k = min(len(pairs), n) if n >= len(pairs) else min(8, n)
    g[:k], u[:k] = [p[0] for p in pairs[:k]], [p[1] for p in pairs[:k]]
    well[:k] = False
    if n >= 1024:                                                  # |silu(g) * up| beyond 448 and beyond 57 344
        u[k:k + 128] = _bits(o.bf16_to_f32(u[k:k + 128]) * np.float32(3000.0))
        g[k:k + 128] = _bits(np.abs(o.bf16_to_f32(g[k:k + 128])) + np.float32(4.0))
        u[k + 128:k + 256] = _bits(o.bf16_to_f32(u[k + 128:k + 256]) * np.float32(1e6))
        well[k:k + 256] = False
        k += 256
    patterns = n >= 2 ** 18
    if patterns:
        g[k:k + 65536] = o.all_bf16_patterns()
        u[k + 65536:k + 131072] = o.all_bf16_patterns()
        well[k:k + 131072] = False
    return {"gate": gate, "up": up, "well": well.reshape(rows, cols), "patterns": patterns}


def strided(bits, row_stride):
    """[rows, cols] -> the rows as a column slice of a [rows, row_stride] buffer whose other columns hold NaN."""
    rows, cols = bits.shape
    buf = np.full((rows, row_stride), NAN, U16)
    buf[:, :cols] = bits
    return buf


# ---- GELU -------------------------------------------------------------------------------------------------------------------------------
GELU_PLANTS = (0x0000, NEG_ZERO, POS_INF, NEG_INF, NAN, MAX, NEG_MAX, SUBNORMAL, 0x8001, MIN_NORMAL, 0xC0B4, 0xC170, 0x4170, 0x43E8, 0x4768, 0xC768)
GELU_SIGMA = 1.5


def gelu_case(n):
    """dict(x [n] patterns, well, patterns).  8 elements: the first eight planted values only."""
    rng = np.random.default_rng(_seed("gelu", n))
    x = _normal(rng, (n,), GELU_SIGMA)
    well = np.ones(n, bool)
    k = min(len(GELU_PLANTS), n)
    x[:k] = GELU_PLANTS[:k]
    well[:k] = False
    patterns = n >= 2 ** 18
    if patterns:
        x[k:k + 65536] = o.all_bf16_patterns()
        well[k:k + 65536] = False
    return {"x": x, "well": well, "patterns": patterns}


def weight_case(n):
    """[n] patterns of a weight, N(0, 0.1), exact zeros, all patterns where they fit."""
    rng = np.random.default_rng(_seed("weight", n))
    w = _normal(rng, (n,), 0.1)
    w[::1013] = 0
    if n >= 8 + 65536:
        w[8:8 + 65536] = o.all_bf16_patterns()
    return w


# ---- the shapes the GPU tests launch (tests/test_gpu_elementwise_ops.py explains each) -----------------------------------------------------
ROPE_SHAPES = ((2, 5, 3, 1, 16), (3, 77, 8, 2, 64), (1, 9, 2, 2, 48), (2, 33, 4, 4, 128))
ROPE_PAST_CLAMP = (1, 3301, 32, 8, 128)
# (Hq, Hk, D, token counts): nv_max = Hq D / 8 = 2, 24, 96, 254, 256, 320
ROPE_FQ_PACKING = ((1, 1, 16, (385, 511)), (3, 1, 64, (21, 39)), (12, 4, 64, (9,)), (127, 5, 16, (6, 1)), (16, 2, 128, (6, 1)), (20, 4, 128, (6, 1)))
ROPE_FQ_PAST_CLAMP = (1, 16384 + 37, 16, 1, 128)
ROPE_VALUE_PAST_CLAMP = (1, 16512, 16, 1, 128)
SILU_SHAPES = ((1, 8), (3, 16384), (257, 24), (5, 4096))
SILU_PAST_CLAMP = (4100, 4104)
GELU_SIZES = (8, 8 * 257)
GELU_PAST_CLAMP = 8 * (256 * 32 * 256 + 256 * 3 + 5)
SILU_SHARE, GELU_SHARE = 0.99, 0.98
