"""The inputs of the row-reduction kernel tests (tests/test_gpu_row_kernels.py) -- TEST INFRASTRUCTURE ONLY, numpy only.

One small tensor per case whose ROWS are the data regimes, so one launch covers them all.  tests/test_oracle_rows_cpu.py asserts, from
the oracle alone, what the GPU tests rely on for every case built here: the decided share of the well-conditioned rows and the closed-form
values of the degenerate ones.  Rows are addressed by name (`names`, one per row).
"""
import numpy as np

from . import qt_oracle as o

BF16_MIN = 0xFF7F           # the most negative finite bf16: what additive attention masks hold
NEG_INF = 0xFF80
NAN = 0x7FC0
POS_INF = 0x7F80


def _seed(*key):
    """A seed that does not depend on PYTHONHASHSEED."""
    s = 0
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def _bits(a):
    with np.errstate(over="ignore"):
        return o.f32_to_bf16(np.asarray(a, np.float64).astype(np.float32))


# ---- norms ------------------------------------------------------------------------------------------------------------------------------
RMS_COLS = (8, 2048, 4096, 4104, 8192, 8200, 16384)
RMS_REFUSED_COLS = 16392
RMS_VARIANT_COLS = (4096, 4104, 8200)
RMS_ROW_COUNTS = (1, 3)
LN_COLS = (8, 512, 520, 1024, 1032, 4096, 4104, 8192, 8200, 16384)
LN_CONST_COLS = (56, 120, 1000)              # lengths at which sum * (1 / cols) is not the constant
LN_VARIANT_COLS = (1024, 4104, 8200)
LN_ROW_COUNTS = (1, 4, 5)
LN_EPS = (1e-12, 1e-5)
LN_CONSTANTS = (1.0, 3.0, 5.5)               # c * k is exact in fp32 for every k <= 16384: any summation order gives the exact sum
TRAIN_COLS = (8, 512, 520, 1024)
TRAIN_REFUSED_COLS = 1032
TRAIN_ROWS = (1, 8, 9, 257)

# ("n01_x1.37": an N(0, 1) row has r within 2^-9 of 1 at the longer lengths, and a 2^k multiple of it likewise of 2^-k: h = bf16(x * r)
# is then x itself, scaled exactly, and no error in r below 2^-9 relative shows in any element.  At r = 0.73 every error in r moves elements.)
NORM_REGIMES = ("n01_2m60", "n01", "n01_2p40", "zero", "overflow", "one_nan", "one_inf", "n01_x1.37")
LN_EXTRA_REGIMES = ("offset64", "const1", "const3", "const5.5")
# rows the decided-share condition does not cover (checked by the interval only): constant rows and rows with |mean| / std >= 32 --
# the radius of the mean, squared, is not small against their variance + eps
LN_ILL_CONDITIONED = ("offset64", "const1", "const3", "const5.5")
NOT_FINITE = ("one_nan", "one_inf")


def _norm_row(name, cols, rng):
    n = rng.standard_normal(cols)
    if name == "n01_2m60":
        return n * 2.0 ** -60
    if name == "n01":
        return n
    if name == "n01_2p40":
        return n * 2.0 ** 40
    if name == "n01_x1.37":
        return n * (1.37 / np.sqrt((n * n).mean()))              # rms 1.37 whatever the sample: r = 0.730, near no short binary fraction
    if name == "zero":
        return np.zeros(cols)
    if name == "overflow":                                        # every |x| >= 2^64: every square is beyond the fp32 maximum
        return np.sign(n) * 2.0 ** 64 * (1 + np.abs(n))
    if name == "one_nan":
        n[cols // 2] = np.nan
        return n
    if name == "one_inf":
        n[cols - 1] = np.inf
        return n
    if name == "offset64":
        return 64 + n
    if name.startswith("const"):
        return np.full(cols, float(name[5:]))
    raise KeyError(name)


def _split(name, target, rng):
    """(h, r) bf16 patterns with bf16(h + r) in the regime of `target`: exactly zero / constant for those rows."""
    cols = target.shape[0]
    if name == "zero":
        h = _bits(rng.standard_normal(cols))
        return h, h ^ np.uint16(0x8000)
    if name.startswith("const"):
        k = rng.integers(-8, 9, cols) * 0.25                     # c / 2 +- k: exact in bf16, and so is their sum c
        return _bits(target / 2 + k), _bits(target / 2 - k)
    with np.errstate(invalid="ignore", over="ignore"):
        h = o.bf16_to_f32(_bits(target * rng.uniform(0.25, 0.75, cols))).astype(np.float64)
        r = np.where(np.isfinite(target), target - h, 1.0)
    return _bits(h), _bits(r)


def norm_case(kind, cols, residual=False, names=None):
    """kind 'rms' / 'ln'.  Returns dict(names, x, res (or None), w, b): bf16 patterns, x / res [rows, cols]."""
    names = tuple(names) if names is not None else NORM_REGIMES + (LN_EXTRA_REGIMES if kind == "ln" else ())
    rng = np.random.default_rng(_seed(kind, cols, residual))
    xs, rs = [], []
    for nm in names:
        t = _norm_row(nm, cols, rng)
        if residual:
            h, r = _split(nm, t, rng)
            xs.append(h)
            rs.append(r)
        else:
            xs.append(_bits(t))
    w = _bits(1 + 0.1 * rng.standard_normal(cols))
    b = _bits(0.1 * rng.standard_normal(cols) + 0.02)
    return dict(names=names, x=np.stack(xs), res=np.stack(rs) if residual else None, w=w, b=b)


def well_conditioned(names):
    return np.array([n not in LN_ILL_CONDITIONED and n not in NOT_FINITE for n in names])


TRAIN_REGIMES = ("n01_2m60", "n01", "n01_2p40", "zero", "overflow", "offset64", "const1", "const3", "const5.5")


def train_case(rows, cols, residual=False):
    """The training LayerNorm's input: the finite regimes in turn (a NaN would spread over every column sum of the backward), and dy."""
    names = tuple(TRAIN_REGIMES[i % len(TRAIN_REGIMES)] for i in range(rows))
    c = norm_case("ln_train%d" % rows, cols, residual, names)
    rng = np.random.default_rng(_seed("dy", rows, cols))
    c["dy"] = _bits(rng.standard_normal((rows, cols)) * 2.0 ** -10)
    return c


# ---- softmax ----------------------------------------------------------------------------------------------------------------------------
SOFTMAX_COLS = (8, 128, 136, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4096)
SOFTMAX_REFUSED_COLS = 4104
SOFTMAX_LIVE_COLS = (8, 136, 264, 520, 1032, 2056)
SOFTMAX_SCALINGS = (0.125, 0.08838834764831845)
SOFTMAX_MASKS = ("none", "per_bq", "per_b")
SOFTMAX_BWD_COLS = (8, 128, 136, 256, 264, 512, 520, 1024, 1032, 2048)
SOFTMAX_BWD_REFUSED_COLS = 2056
SCORE_REGIMES = ("n03", "n040", "all_equal", "dominant", "dominant_subnormal", "dominant_dead", "one_nan")
MASK_REGIMES = ("fully_masked", "first_live", "last_live", "trailing_vectors", "neginf_part", "neginf_row")
# rows outside the decided-share condition: probabilities in the fp32 subnormal range carry the absolute flush allowance, which spans
# many bf16 steps down there.  (The all-NaN rows, "one_nan" and "mask_neginf_row", have no finite element to count; "dominant_dead" is
# decided throughout -- exact zeros around an exact 1 -- and counts.)
SOFTMAX_EXEMPT = ("dominant_subnormal",)


def softmax_rows_per_group(cols):
    """(lanes per row, the ragged / single-group row counts the issue asks for)."""
    if cols <= 128:
        return 16, (1, 17)
    if cols <= 256:
        return 32, (9,)
    return 64, (5,)


def _score_row(name, cols, scaling, rng):
    n = rng.standard_normal(cols)
    if name == "n040":
        return n * 40
    if name == "all_equal":
        return np.full(cols, 2.5)
    s = n * 3
    if name.startswith("dominant"):
        # the other probabilities: ordinary / in the fp32 subnormal range (exp(-95) = 5e-42) / on both sides of the kernel's
        # skip-this-vector threshold (110 below the maximum)
        s[cols // 3] += {"dominant": 30.0, "dominant_subnormal": 95.0, "dominant_dead": 110.0}[name] / scaling
    if name == "one_nan":
        s[cols // 2] = np.nan
    return s


def softmax_case(cols, scaling, mask_kind):
    """Scores [B = 2, H = 2, Q, cols] and an additive mask ([B, 1, Q, cols], [B, 1, 1, cols] or None) as bf16 patterns.  Returns
    dict(names [B * H * Q], scores, mask, B, H, Q, strides (sb, sh, sq))."""
    rng = np.random.default_rng(_seed("softmax", cols, scaling, mask_kind))
    B, H = 2, 2
    names = SCORE_REGIMES + (tuple("mask_" + m for m in MASK_REGIMES) if mask_kind == "per_bq" else ())
    Q = len(names)
    scores = np.empty((B, H, Q, cols), np.uint16)
    for bh in range(B * H):
        for q, nm in enumerate(names):
            scores[bh // H, bh % H, q] = _bits(_score_row(nm if not nm.startswith("mask_") else "n03", cols, scaling, rng))
    mask, strides = None, (0, 0, 0)
    if mask_kind == "per_bq":
        mask = np.zeros((B, 1, Q, cols), np.uint16)
        for q, nm in enumerate(names):
            if not nm.startswith("mask_"):
                if q % 2:
                    mask[:, 0, q, cols - cols // 4:] = BF16_MIN    # an ordinary padded tail under the score regimes too
                continue
            m = nm[5:]
            if m == "fully_masked":
                mask[:, 0, q, :] = BF16_MIN
            elif m == "first_live":
                mask[:, 0, q, 1:] = BF16_MIN
            elif m == "last_live":
                mask[:, 0, q, :-1] = BF16_MIN
            elif m == "trailing_vectors":
                mask[:, 0, q, max(8 * (cols // 24), min(8, cols - 1)):] = BF16_MIN
            elif m == "neginf_part":
                mask[:, 0, q, cols // 2:] = NEG_INF
            elif m == "neginf_row":
                mask[:, 0, q, :] = NEG_INF
        strides = (Q * cols, 0, cols)
    elif mask_kind == "per_b":
        mask = np.zeros((B, 1, 1, cols), np.uint16)
        mask[0, 0, 0, cols - cols // 3:] = BF16_MIN
        mask[1, 0, 0, cols // 2:] = BF16_MIN
        strides = (cols, 0, 0)
    return dict(names=tuple(names) * (B * H), scores=scores, mask=mask, B=B, H=H, Q=Q, strides=strides)


def softmax_share_rows(names):
    return np.array([n not in SOFTMAX_EXEMPT for n in names])


def softmax_bwd_case(cols, dp_std):
    """P [rows, cols] from the oracle's forward (N(0, 3) scores, a padded tail on some rows), one-hot rows and uniform rows; dP ~ N(0,
    dp_std).  Returns dict(names, p, dp, scaling)."""
    rng = np.random.default_rng(_seed("softmax_bwd", cols, dp_std))
    scaling = 0.125
    names = ("softmax",) * 12 + ("one_hot",) * 3 + ("uniform",) * 3
    sc = _bits(rng.standard_normal((12, cols)) * 3 / scaling)
    mask = np.zeros((12, cols), np.uint16)
    mask[::3, cols - cols // 4:] = BF16_MIN
    p = np.zeros((len(names), cols), np.uint16)
    p[:12] = o.softmax_fq(sc, mask, scaling, None)[0]
    for i, k in enumerate((0, cols // 2, cols - 1)):
        p[12 + i, k] = 0x3F80
    p[15:] = _bits(1.0 / cols)
    dp = rng.standard_normal(p.shape) * dp_std
    # (few-bit data under a uniform P puts (dP - dot) / cols exactly ON bf16 ties at short rows, where no radius decides anything: one
    # small entry per row gives the dot product low-order bits)
    dp[15:, 1] *= 2.0 ** -6
    dp = _bits(dp)
    return dict(names=names, p=p, dp=dp, scaling=scaling)


# ---- causal-LM loss ---------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = ((1, 2, 7, 8), (1, 3, 8, 8), (2, 5, 2051, 2056), (1, 4, 2056, 2056), (1, 1, 8, 8))       # (B, S, V, row stride)
LOSS_REGIMES = ("label_col0", "label_last", "label_on_dominant", "label_off_dominant", "all_equal", "first8_neginf", "one_posinf",
                "all_ignored")


def loss_case(shape, regime):
    """Returns dict(logits [B, S, stride] bf16 patterns (columns >= V hold NaN: never to be read), labels [B, S] int64) or None where
    the regime does not exist at that shape."""
    B, S, V, stride = shape
    rng = np.random.default_rng(_seed("loss", shape, regime))
    x = rng.standard_normal((B, S, stride)) * 4
    labels = rng.integers(0, V, (B, S))
    if regime == "label_col0":
        labels[:] = 0
    elif regime == "label_last":
        labels[:] = V - 1
    elif regime in ("label_on_dominant", "label_off_dominant"):
        x[:] = -80.0
        dom = rng.integers(0, V, (B, S))
        np.put_along_axis(x, dom[..., None], 80.0, -1)
        # position s is scored against labels[s + 1]
        labels[:, 1:] = dom[:, :-1] if regime == "label_on_dominant" else (dom[:, :-1] + 1) % V
    elif regime == "all_equal":
        x[:] = 1.5
    elif regime == "first8_neginf":
        if V <= 8:
            return None
        x[..., :8] = -np.inf
        labels[:] = np.maximum(labels, 8)
    elif regime == "one_posinf":
        x[..., V // 2] = np.inf
    elif regime == "all_ignored":
        labels[:] = -100
    if regime != "all_ignored" and S > 2:
        labels[0, 1] = -100                                       # one ignored label among the scored ones
    bits = _bits(x)
    bits[..., V:] = NAN
    return dict(logits=bits, labels=labels.astype(np.int64))
