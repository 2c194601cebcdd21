"""The inputs of the attention-core kernel tests (tests/test_gpu_attention_cores.py) -- TEST INFRASTRUCTURE ONLY, numpy only.

One list of named cases per kernel family, shared by the CPU test of the oracle (tests/test_oracle_attention_cpu.py: what the GPU test
relies on -- exact score sums, the decided shares, the containment of oracle.attention_fq and of torch's own chain) and by the GPU test.

Values: q and k are integers in [-8, 8] (head_dim 64) or [-4, 4] (head_dim 128) times 2^-2, v integers in [-8, 8] times 2^-2, so every
score sum and -- on the 8-bit grids -- every P'.V sum is exact in fp32 in any order (oracle.attention_interval).  Off-grid v (one case per
kernel that quantizes v itself) is N(0, 1) in bf16.  The FP8 core's v holds one key per column (see fp8_cases).  Seeds are fixed by the case's name.  Shapes are the smallest that reach a branch;
`branch` names it.
"""
import numpy as np

from . import qt_oracle as o
from .row_cases import BF16_MIN, NAN, NEG_INF, POS_INF, _seed

U16 = np.uint16
POISON = POS_INF                 # what the padding between mask rows holds (a stride of Sk + 4): a kernel that reads it shows
DEFAULT_CUS = 256                # compute units of the MI355X; the GPU test passes the device's own count


def _bits(a):
    return o.f32_to_bf16(np.asarray(a, np.float64).astype(np.float32))


class Case:
    """One launch problem.  q, k, v: uint16 [B, H, S, D] bf16 patterns (v as handed to the value pass: unquantized where v_offgrid).
    mask: uint16 [mb, mh, mq, Sk] with mb in (1, B), mh in (1, H), mq in (1, Sq), or None; row_stride: elements between mask rows.
    fmt: the probabilities' format name or None; form: "plain" (the map / closed form as format_for gives it), "rows" (table format
    with the row words); scale: None (unit, no scale tensor) or a float (the device scale); obs: the observer's amax slot is passed.
    out_fq: the launch forms with the consumer's fake-quantizer are checked too.  live: the row-extent launch forms are checked too.
    readout: first key of the identity window of V (P' read-out case) or None."""

    def __init__(self, name, family, q, k, v, mask=None, row_stride=None, fmt=None, form="plain", scale=None, obs=False, out_fq=False, live=False,
                 readout=None, branch="", v_offgrid=False):
        self.name, self.family = name, family
        self.q, self.k, self.v = q, k, v
        self.B, self.H, self.Sq, self.D = q.shape
        self.Sk = k.shape[2]
        self.mask, self.row_stride = mask, (row_stride or self.Sk)
        self.fmt, self.form, self.scale, self.obs, self.out_fq, self.live = fmt, form, scale, obs, out_fq, live
        self.readout, self.branch, self.v_offgrid = readout, branch, v_offgrid
        self.scaling = float(self.D) ** -0.5
        self.kernel = {"fq": "online", "rows": "strip", "fp8": "strip_fp8"}[family]

    def __repr__(self):
        return self.name

    # ---- what the launches need -----------------------------------------------------------------------------------------------------------
    def mask_strides(self):
        """(mask_sb, mask_sh, mask_sq) in elements; 0 for a broadcast dimension."""
        if self.mask is None:
            return 0, 0, 0
        mb, mh, mq, _ = self.mask.shape
        rs = self.row_stride
        return (mh * mq * rs if mb > 1 else 0), (mq * rs if mh > 1 else 0), (rs if mq > 1 else 0)

    def live_strides(self):
        """(live_sb, live_sh, live_sq) in mask rows."""
        mb, mh, mq, _ = self.mask.shape
        return (mh * mq if mb > 1 else 0), (mq if mh > 1 else 0), (1 if mq > 1 else 0)

    def mask_rows(self):
        mb, mh, mq, _ = self.mask.shape
        return mb * mh * mq

    def mask_buffer(self):
        """The mask as it lies in memory: rows row_stride apart, POISON between them (nothing may read it)."""
        rows = self.mask.reshape(-1, self.Sk)
        buf = np.full((rows.shape[0], self.row_stride), POISON, U16)
        buf[:, :self.Sk] = rows
        return buf.reshape(-1)

    def extents(self):
        """(row_live int32 [mask rows], irregular) as qt_mask_row_live_checked defines them: one past the last column above -1e30;
        irregular = some row is not exactly "zeros, then the bf16 minimum"."""
        rows = self.mask.reshape(-1, self.Sk)
        with np.errstate(invalid="ignore"):
            above = o.bf16_to_f32(rows) > -1e30
        ext = np.where(above.any(axis=1), self.Sk - np.argmax(above[:, ::-1], axis=1), 0).astype(np.int32)
        cols = np.arange(self.Sk)[None, :]
        regular = np.where(cols < ext[:, None], rows == 0, rows == BF16_MIN).all()
        return ext, int(not regular)

    # ---- what the oracle needs -------------------------------------------------------------------------------------------------------------
    def qmap(self):
        return o.get_quantization_map(self.fmt) if self.fmt else None

    def scale_bits(self):
        return None if self.scale is None else o.f32_to_bf16(np.float32(self.scale))

    def vq(self):
        """fq_v(v): what the attention core multiplies by.  The rows and fp8 families quantize v in their value pass (a v that is
        already on the format's grid stays; [-8, 8] / 4 is not on fp4_e2m1's); the two-pass core takes v as it is."""
        return o.canon_nan16(o.vmap_bf16(self.v, self.qmap())) if self.family != "fq" else self.v

    def intervals(self, out_fq=False):
        key = (self.name, bool(out_fq), self.B)
        if key not in _INTERVALS:
            _INTERVALS[key] = o.attention_interval(self.q, self.k, self.vq(), self.mask, self.scaling, self.qmap(), self.scale_bits(),
                                                   self.qmap() if out_fq else None, kernel=self.kernel)
        return _INTERVALS[key]


_INTERVALS = {}


# ---- values -------------------------------------------------------------------------------------------------------------------------------
def _qkv(name, B, H, Sq, Sk, D, v_offgrid=False):
    rng = np.random.default_rng(_seed("attention", name))
    top = 8 if D == 64 else 4
    q = _bits(rng.integers(-top, top + 1, (B, H, Sq, D)) * 0.25)
    k = _bits(rng.integers(-top, top + 1, (B, H, Sk, D)) * 0.25)
    v = _bits(rng.standard_normal((B, H, Sk, D))) if v_offgrid else _bits(rng.integers(-8, 9, (B, H, Sk, D)) * 0.25)
    return q, k, v, rng


def one_key_per_column(v):
    """v with every column d of head h kept at ONE key, (37 d + 11 h + 5) mod Sk, and zero elsewhere: O[d] is then one exact product
    P'[key] x v[key, d] -- the keys of a head's columns spread over every key block, tile and lane group."""
    B, H, Sk, D = v.shape
    keep = np.zeros((H, Sk, D), bool)
    d = np.arange(D)
    for h in range(H):
        keep[h, (37 * d + 11 * h + 5) % Sk, d] = True
    return np.where(keep[None], v, U16(0)).astype(U16)


def _identity_v(B, H, Sk, D, first):
    v = np.zeros((B, H, Sk, D), U16)
    v[:, :, first + np.arange(D), np.arange(D)] = 0x3F80            # 1.0
    return v


# ---- masks: uint16 [mb, mh, mq, Sk] -------------------------------------------------------------------------------------------------------
def causal(Sq, Sk):
    m = np.where(np.arange(Sk)[None, :] > np.arange(Sq)[:, None], U16(BF16_MIN), U16(0)).astype(U16)
    return m[None, None]


def from_extents(ext, Sk, fill=BF16_MIN):
    """Rows "zeros, then `fill`" with the given extents; any leading shape."""
    ext = np.asarray(ext)
    return np.where(np.arange(Sk) < ext[..., None], U16(0), U16(fill)).astype(U16)


def padding(exts, Sk):
    return from_extents(np.asarray(exts), Sk)[:, None, None, :]


def ragged(Sq, Sk, rng):
    """[1, 1, Sq, Sk] rows "zeros, then the minimum" with extents that are no multiple of anything, 0 (no unmasked key) and Sk included."""
    ext = rng.integers(0, Sk + 1, Sq)
    ext[0] = Sk
    if Sq > 2:
        ext[1], ext[Sq // 2] = 0, 0
    return from_extents(ext, Sk)[None, None]


def bias(shape, rng):
    return _bits(rng.standard_normal(shape) * 2.0)


def hole(Sq, Sk, lo, hi, rng=None):
    m = np.zeros((1, 1, Sq, Sk), U16) if rng is None else bias((1, 1, Sq, Sk), rng)
    m[..., lo:hi] = BF16_MIN
    return m


def redo(Sq, Sk, fill, row):
    """Keys 64 .. 127 masked for every row (a dead tile), and `row` masked everywhere."""
    m = np.zeros((1, 1, Sq, Sk), U16)
    m[..., 64:128] = fill
    m[0, 0, row, :] = fill
    return m


# ---- the fused two-pass core: qt_attention_fq_bf16 / _live_bf16 / _out_bf16 (csrc/qt_attention.hip) ---------------------------------------
def fq_cases(cus=DEFAULT_CUS):
    out = []

    def add(name, B, H, Sq, Sk, D, mask=None, **kw):
        q, k, v, rng = _qkv(name, B, H, Sq, Sk, D)
        m = mask(rng) if callable(mask) else mask
        out.append(Case(name, "fq", q, k, v, m, **kw))
        return out[-1]

    add("sq1_sk4_d64_none", 1, 2, 1, 4, 64, obs=True, branch="Sk < 64, Sq = 1, QT_FMT_IDENTITY, no mask")
    add("sq63_sk12_d64_none_ragged", 1, 2, 63, 12, 64, mask=lambda r: ragged(63, 12, r), live=True, obs=True,
        branch="Sk < 64 with a mask; extents incl. 0 through row_live; scalar scan (Sk % 8 != 0)")
    add("sq64_sk60_d64_e5m2_padding", 2, 3, 64, 60, 64, mask=padding([60, 17], 60), fmt="e5m2", live=True, out_fq=True,
        branch="[B,1,1,Sk] right padding; e5m2 hardware conversion (p8 = 2); out_fq")
    add("sq65_sk64_d64_e4m3_s2m1_bhqk", 2, 2, 65, 64, 64, mask=lambda r: bias((2, 2, 65, 64), r), fmt="e4m3", scale=0.5, obs=True,
        branch="!UNIT (power-of-two scale); [B,H,Sq,Sk] mask, mask_sh != 0; Sq = 65; vector scan")
    add("sq130_sk68_d128_e4m3_s037_stride", 1, 2, 130, 68, 128, mask=lambda r: ragged(130, 68, r), row_stride=72, fmt="e4m3", scale=0.37, live=True,
        branch="!UNIT (0.37); rows Sk + 4 apart; scalar scan (Sk % 8 != 0); Sq = 130; ragged last tile")
    add("sq65_sk64_d64_e4m3_stride68", 1, 2, 65, 64, 64, mask=lambda r: ragged(65, 64, r), row_stride=68, fmt="e4m3", live=True,
        branch="Sk % 8 == 0 with a row stride of Sk + 4, no multiple of 8: the scalar scan by the stride alone")
    add("sq65_sk128_d64_int8_s2m7_bias", 1, 3, 65, 128, 64, mask=lambda r: bias((1, 1, 65, 128), r), fmt="int8", scale=2.0 ** -7, obs=True, live=True,
        branch="QT_FMT_INT, !UNIT (2^-7); finite random bias: the irregular flag keeps the live form on the mask")
    add("sq64_sk200_d128_int8_s0079_causal", 1, 2, 64, 200, 128, mask=causal(64, 200), fmt="int8", scale=0.0079, live=True,
        branch="QT_FMT_INT, !UNIT (0.0079); causal: dead suffix tiles skipped; Sk = 200")
    add("sq130_sk200_d64_posit8_1_hole", 1, 2, 130, 200, 64, mask=hole(130, 200, 64, 128), fmt="posit8_1", live=True,
        branch="QT_FMT_LUT plain map; a dead tile that is not a suffix (keys 64 .. 127)")
    add("sq65_sk128_d128_posit8_1_rows_padding", 2, 2, 65, 128, 128, mask=padding([128, 40], 128), fmt="posit8_1", form="rows", live=True, out_fq=True,
        obs=True, branch="kFmtRows; right padding; out_fq through the row form")
    add("sq64_sk128_d64_e4m3_redo_min", 1, 2, 64, 128, 64, mask=redo(64, 128, BF16_MIN, 37), fmt="e4m3", obs=True,
        branch="a dead tile skipped, then 'some row is masked everywhere': every tile counted again (uniform row)")
    add("sq64_sk128_d64_e4m3_redo_inf", 1, 2, 64, 128, 64, mask=redo(64, 128, NEG_INF, 37), fmt="e4m3",
        branch="the same with -inf: the row is NaN, as torch's softmax gives")
    add("sq1_sk4100_d64_e4m3_padding", 1, 2, 1, 4100, 64, mask=padding([3000], 4100), fmt="e4m3", obs=True,
        branch="ntiles = 65 > 64: skipping off")
    add("sq8_sk64_d64_e4m3_snake", cus + 1, 1, 8, 64, 64, mask=lambda r: padding(r.integers(1, 65, cus + 1), 64), fmt="e4m3", live=True,
        branch="snake order: CUs + 1 workgroups, not a multiple of twice the CU count")
    add("sq130_sk200_d128_e4m3_nomask", 1, 2, 130, 200, 128, fmt="e4m3", obs=True, branch="e4m3 hardware conversion (p8 = 1); no mask; three query blocks")
    c = add("sq65_sk64_d64_e4m3_nan_query", 1, 2, 65, 64, 64, fmt="e4m3", branch="one NaN query row: that row is NaN, the workgroup's others are not")
    c.q[0, 1, 20, :] = NAN
    c = add("sq65_sk128_d64_e4m3_inf_key", 1, 2, 65, 128, 64, mask=causal(65, 128), fmt="e4m3",
            branch="one +inf key element: rows with q > 0 or q = 0 there are NaN, rows with q < 0 give that key probability 0")
    c.k[0, 0, 5, 3] = POS_INF
    # P' read-out: V is the identity on keys 32 .. 95 (both tiles), zero elsewhere
    q, k, _, rng = _qkv("readout_fq", 1, 2, 65, 128, 64)
    out.append(Case("sq65_sk128_d64_e4m3_readout", "fq", q, k, _identity_v(1, 2, 128, 64, 32), fmt="e4m3", readout=32, obs=True,
                    branch="P' read-out: the output is P' of keys 32 .. 95"))
    return out


# ---- the table-format core with the strip in registers: qt_value_t_rows + qt_attention_rows_bf16 (csrc/qt_attention_rows.hip) ---------------
def rows_cases():
    out = []

    def add(name, B, H, Sq, Sk, mask=None, v_offgrid=False, **kw):
        q, k, v, rng = _qkv(name, B, H, Sq, Sk, 128, v_offgrid)
        m = mask(rng) if callable(mask) else mask
        out.append(Case(name, "rows", q, k, v, m, form="rows", out_fq=True, v_offgrid=v_offgrid, **kw))

    add("sq1_sk128_posit8_1_nomask", 1, 2, 1, 128, fmt="posit8_1", branch="Sq = 1, one key block, MODE 0")
    add("sq64_sk256_posit8_2_ragged", 1, 2, 64, 256, mask=lambda r: ragged(64, 256, r), fmt="posit8_2", live=True,
        branch="extents incl. 0 (a row with no unmasked key): MODE 1, and the mask read in full: MODE 2")
    add("sq65_sk1024_fp4_bhqk", 1, 2, 65, 1024, mask=lambda r: bias((1, 2, 65, 1024), r), fmt="fp4_e2m1", branch="eight key blocks; [1,H,Sq,Sk] mask, mask_sh != 0; Sq = 65")
    add("sq130_sk256_posit8_1_hole", 1, 2, 130, 256, mask=hole(130, 256, 64, 192), fmt="posit8_1", live=True,
        branch="the irregular flag with extents: the mask is read inside them; Sq = 130")
    add("sq65_sk128_posit8_2_offgrid_padding", 2, 2, 65, 128, mask=padding([77, 0], 128), fmt="posit8_2", v_offgrid=True, live=True,
        branch="qt_value_t_rows quantizes v; a batch with no unmasked key (uniform rows)")
    q, k, _, rng = _qkv("readout_rows", 1, 2, 64, 256, 128)
    out.append(Case("sq64_sk256_posit8_1_readout", "rows", q, k, _identity_v(1, 2, 256, 128, 96), form="rows", fmt="posit8_1", readout=96,
                    branch="P' read-out: the output is P' of keys 96 .. 223 (both key blocks, both wave groups)"))
    return out


# ---- the FP8 core: qt_value_codes_t + qt_attention_fp8 (csrc/qt_attention_fp8.hip) ----------------------------------------------------------
# Its P'.V runs on the scaled matrix instruction, whose sum of several products that span many binades cannot be pinned (oracle.
# attention_interval, "strip_fp8"), so v holds ONE key per column (one_key_per_column): every output element is one exact product, decided
# wherever P' is, and still shows a wrong probability, a wrong key order of V^T and a wrong mask form.  The value pass itself is checked on
# a dense v by the GPU test.
def fp8_cases():
    out = []

    def add(name, B, H, Sq, Sk, D, fmt, mask=None, v_offgrid=False, **kw):
        q, k, v, rng = _qkv(name, B, H, Sq, Sk, D, v_offgrid)
        m = mask(rng) if callable(mask) else mask
        out.append(Case(name, "fp8", q, k, one_key_per_column(v), m, fmt=fmt, v_offgrid=v_offgrid, **kw))

    add("sq1_sk128_d64_e4m3_bhqk", 1, 2, 1, 128, 64, "e4m3", mask=lambda r: bias((1, 2, 1, 128), r), branch="head_dim 64 (MB = 4); Sq = 1; mask_sh != 0: MODE 2")
    add("sq65_sk128_d128_e5m2_hole", 1, 2, 65, 128, 128, "e5m2", mask=hole(65, 128, 32, 96), live=True, branch="a hole: irregular, read inside the extents; Sq = 65")
    add("sq130_sk256_d128_e4m3_offgrid_ragged", 1, 2, 130, 256, 128, "e4m3", mask=lambda r: ragged(130, 256, r), v_offgrid=True, live=True,
        branch="qt_value_codes_t quantizes v; extents incl. 0 (rows with no unmasked key): MODE 1 by mask_is_simple and by the device flag")
    add("sq130_sk256_d64_e5m2_ragged", 1, 2, 130, 256, 64, "e5m2", mask=lambda r: ragged(130, 256, r), live=True, branch="head_dim 64; the same extents forms")
    add("sq65_sk128_d64_e4m3_padding0", 2, 1, 65, 128, 64, "e4m3", mask=padding([128, 0], 128), live=True, branch="a batch with no unmasked key")
    q, k, _, rng = _qkv("readout_fp8", 1, 2, 65, 128, 128)
    out.append(Case("sq65_sk128_d128_e4m3_readout", "fp8", q, k, _identity_v(1, 2, 128, 128, 0), fmt="e4m3", readout=0, branch="P' read-out: the output is P' of all 128 keys"))
    return out


def all_cases(cus=DEFAULT_CUS):
    return fq_cases(cus) + rows_cases() + fp8_cases()


# ---- what the refusal tests pass ----------------------------------------------------------------------------------------------------------
FQ_REFUSED_SK = 62                 # Sk % 4 != 0
FQ_REFUSED_D = 32
REFUSED_BH = 65536
FQ_REFUSED_MASK_STRIDE = 66        # not a multiple of 4
ROWS_REFUSED_SK = (64, 1152)
