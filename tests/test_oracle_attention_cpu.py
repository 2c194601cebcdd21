"""What tests/test_gpu_attention_cores.py relies on, checked from the oracle alone (no GPU): for every case of oracle/attention_cases.py

  * the premise of oracle.attention_interval holds (exact score sums: it raises otherwise) and, on the grids it is stated for, the
    P'.V sums carry no radius;
  * the interval contains oracle.attention_fq (the fp64 restatement pinned to upstream by tests/test_oracle_golden.py) and, at unit
    scale, torch's own CPU bf16 module chain (modules/quantizable/modeling_bert.py:118-158);
  * THE CAP: at least 95 % of the finite output elements of EVERY case are decided (lo == hi), and at least 99.9 % of the P' elements
    of a read-out case and of every case of the FP8 core (whose v holds one key per column: its outputs are single products).  This is a condition on the INPUTS: a case that misses it is changed,
    never the cap;
  * the NaN rows are exactly the ones the case is built for;
  * the interval check is sharp: four one-key mistakes applied to attention_fq's output all fall outside it.

Run with -s for the decided shares per case.
"""
import numpy as np
import pytest
import torch

from oracle import attention_cases as ac
from oracle import qt_oracle as o

CASES = ac.all_cases()
IDS = [f"{c.family}-{c.name}" for c in CASES]
EXACT_GRIDS = ("e4m3", "e5m2", "posit8_1", "fp4_e2m1")
CAP, READOUT_CAP = 0.95, 0.999


def _pow2(x):
    return x is not None and float(np.frexp(x)[0]) == 0.5


def test_names_are_unique_and_every_case_names_its_branch():
    assert len(set(IDS)) == len(IDS)
    assert all(c.branch for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_interval_contains_attention_fq_and_meets_the_cap(c):
    iv = c.intervals()                                            # (raises if a score sum is not exact)
    ref, pq = o.attention_fq(c.q, c.k, c.vq(), c.mask, c.scaling, c.qmap(), c.scale_bits())
    assert int(iv.out.distance(ref).max()) == 0, iv.out.report(ref)
    assert int(iv.probs.distance(pq).max()) == 0, iv.probs.report(pq)
    share, pshare = iv.out.decided_share(), iv.probs.decided_share()
    print(f"\n[attention] {c.family} {c.name}: O decided {share:.4f}, P' decided {pshare:.5f}, rows with exact P'.V {iv.pv_exact.mean():.3f}")
    assert share >= CAP, share
    if c.readout is not None or c.family == "fp8":
        assert pshare >= READOUT_CAP, pshare
    if c.readout is not None:
        window = iv.probs.rows((Ellipsis, slice(c.readout, c.readout + c.D)))
        assert window.decided_share() >= 0.999, window.decided_share()
        # ... and the output IS that window: one exact product per element
        assert np.array_equal(iv.out.lo, window.lo) and np.array_equal(iv.out.hi, window.hi)
    if ((c.fmt in EXACT_GRIDS and c.scale is None) or (c.fmt == "int8" and _pow2(c.scale))):
        assert iv.pv_exact[~iv.out.nan.all(axis=-1)].all(), "the P'.V sums of this grid are exact in fp32"
    # with the consumer's map on the way out: the image of the same interval
    if c.out_fq:
        ivq = c.intervals(out_fq=True)
        assert np.array_equal(ivq.out.lo, o.canon_nan16(o.vmap_bf16(iv.out.lo, c.qmap()))) and np.array_equal(ivq.out.hi, o.canon_nan16(o.vmap_bf16(iv.out.hi, c.qmap())))
    # the amax slot: the largest probability in front of fq_P
    if not iv.probs.nan.any():
        p_bits, _ = o.softmax_fq(o.f32_to_bf16(np.einsum("bhqd,bhkd->bhqk", o._b64(c.q), o._b64(c.k)).astype(np.float32)), c.mask, c.scaling, None)
        assert int(iv.amax.distance(np.array([p_bits.max()], np.uint16)).max()) == 0
    else:
        assert iv.amax.nan.all()


def _torch_chain(c):
    bf = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)      # noqa: E731
    q, k, v = bf(c.q), bf(c.k), bf(c.vq())
    s = torch.matmul(q, k.transpose(-1, -2)) * c.scaling
    if c.mask is not None:
        s = s + bf(c.mask)
    p = torch.softmax(s, dim=-1, dtype=torch.float32).to(torch.bfloat16)
    if c.fmt:
        qmap = torch.from_numpy(c.qmap().view(np.int16))
        p = qmap[(p.view(torch.int16).to(torch.int32) & 0xFFFF).long()].view(torch.bfloat16)
    out = torch.matmul(p, v)
    return out.view(torch.int16).numpy().view(np.uint16), p.view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("c", [c for c in CASES if c.scale is None], ids=[i for i, c in zip(IDS, CASES) if c.scale is None])
def test_interval_contains_torchs_own_bf16_chain(c):
    """matmul, * scaling, + mask, softmax(dtype=float32).to(bf16), the value map, matmul -- torch's CPU kernels on bf16 tensors."""
    iv = c.intervals()
    out, p = _torch_chain(c)
    assert int(iv.probs.distance(p).max()) == 0, iv.probs.report(p)
    assert int(iv.out.distance(out).max()) == 0, iv.out.report(out)


def _nan_rows(c):
    want = np.zeros((c.B, c.H, c.Sq), bool)
    if c.name.endswith("redo_inf"):
        want[:, :, 37] = True
    if c.name.endswith("nan_query"):
        want[0, 1, 20] = True
    if c.name.endswith("inf_key"):                                # +inf x q: +inf (NaN row), NaN (q = 0: NaN row) or -inf (probability 0)
        want[0, 0] = o.bf16_to_f32(c.q[0, 0, :, 3]) >= 0
    return want


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_nan_rows_are_the_ones_the_case_is_built_for(c):
    iv = c.intervals()
    want = _nan_rows(c)
    assert np.array_equal(iv.out.nan.all(axis=-1), want) and np.array_equal(iv.out.nan.any(axis=-1), want)
    if c.name.endswith("inf_key"):
        assert 0 < want[0, 0].sum() < c.Sq, "both kinds of rows in one workgroup"


def test_fully_masked_rows_are_uniform_over_all_keys():
    c = next(c for c in CASES if c.name.endswith("redo_min"))
    iv = c.intervals()
    uniform = o.f32_to_bf16(np.float32(1.0 / c.Sk))
    want = o.vmap_bf16(np.array([uniform], np.uint16), c.qmap())[0]
    assert np.all(iv.probs.lo[:, :, 37] == want) and np.all(iv.probs.hi[:, :, 37] == want)


def test_row_granules_divide_every_admissible_probability():
    """_row_granules against brute force on posit8_2 (the grid with the widest range of steps): every grid value inside a row's
    admissible range is an integer multiple of the row's granule, and the granule is the coarsest power of two of that kind."""
    qmap = o.get_quantization_map("posit8_2")
    grid_bits = qmap[np.arange(0x3F81)]
    grid = np.unique(o._b64(grid_bits))
    grid = grid[grid > 0]
    rng = np.random.default_rng(7)
    lo_i = rng.integers(0, len(grid), (40, 6))
    hi_i = np.minimum(lo_i + rng.integers(0, 3, lo_i.shape), len(grid) - 1)
    plo, phi = grid[lo_i], grid[hi_i]
    plo[::5, 0], phi[::7, 1], plo[::7, 1] = 0.0, 0.0, 0.0          # an element that may be zero; an element that is zero
    g = o._row_granules(grid_bits, plo, phi)
    for r in range(plo.shape[0]):
        first = min([a if a > 0 else grid[0] for a, b in zip(plo[r], phi[r]) if b > 0])
        admissible = grid[grid >= first]
        assert np.all(np.mod(admissible / g[r], 1.0) == 0)
        assert np.any(np.mod(admissible / (2 * g[r]), 1.0) != 0)
    assert np.isinf(o._row_granules(grid_bits, np.zeros((1, 4)), np.zeros((1, 4)))[0])


def test_strip_fp8_takes_one_key_per_column_only():
    c = next(c for c in CASES if c.family == "fp8" and c.readout is not None)
    dense = c.v.copy()
    dense[:, :, :, 0] = 0x3F80
    with pytest.raises(ValueError):
        o.attention_interval(c.q, c.k, dense, c.mask, c.scaling, c.qmap(), kernel="strip_fp8")


def test_a_case_that_breaks_the_premise_raises():
    c = CASES[0]
    q = c.q.copy()
    q[0, 0, 0, 0] = 0x4E80                                          # 2^30 x 0.25 next to 0.25 x 0.25: more than 24 bits
    k = c.k.copy()
    k[..., 0] = 0x3E80
    with pytest.raises(ValueError):
        o.attention_interval(q, k, c.v, None, c.scaling, None)


# ---- sharpness: one-key mistakes -------------------------------------------------------------------------------------------------------------
def _wrong(c, mistake):
    """attention_fq's output with one mistake of the kind a kernel makes."""
    q, k, v, m = c.q, c.k, c.vq().copy(), (None if c.mask is None else np.broadcast_to(c.mask, (c.B, c.H, c.Sq, c.Sk)).copy())
    if mistake == "drop the last key":
        m = np.zeros((c.B, c.H, c.Sq, c.Sk), np.uint16) if m is None else m
        m[..., -1] = ac.BF16_MIN
        return o.attention_fq(q, k, v, m, c.scaling, c.qmap(), c.scale_bits())[0]
    if mistake == "swap two keys of V":
        i, j = (0, 1) if c.family == "fq" else (5, 42)             # (the FP8 core's v: keys that columns 0 and 1 of head 0 read)
        v[:, :, [i, j]] = v[:, :, [j, i]]
        return o.attention_fq(q, k, v, m, c.scaling, c.qmap(), c.scale_bits())[0]
    if mistake == "quantize P with scale 1":
        return o.attention_fq(q, k, v, m, c.scaling, c.qmap(), None)[0]
    if mistake == "a fully masked row takes only the live tiles":
        m[..., 64:] = ac.NEG_INF                                   # the dead tile never counted: the row is uniform over keys 0 .. 63
        return o.attention_fq(q, k, v, m, c.scaling, c.qmap(), c.scale_bits())[0]
    raise KeyError(mistake)


@pytest.mark.parametrize("mistake,family,case", [("drop the last key", "fq", "sq1_sk4_d64_none"), ("swap two keys of V", "fq", "sq1_sk4_d64_none"),
                                                 ("quantize P with scale 1", "fq", "sq65_sk64_d64_e4m3_s2m1_bhqk"),
                                                 ("a fully masked row takes only the live tiles", "fq", "sq64_sk128_d64_e4m3_redo_min"),
                                                 # ... and with one key per column the FP8 core's check still sees the order of V's keys
                                                 ("swap two keys of V", "fp8", "sq1_sk128_d64_e4m3_bhqk")])
def test_the_interval_check_is_sharp(mistake, family, case):
    """Each mistake, applied to attention_fq's output on the smallest case that can show it, fails the `inside` check."""
    c = next(c for c in CASES if c.name == case and c.family == family)
    iv = c.intervals()
    d = iv.out.distance(_wrong(c, mistake))
    print(f"\n[attention] {mistake} on {case}: {int((d > 0).sum())} of {d.size} elements outside, worst {int(d.max())} bf16 steps")
    assert int(d.max()) > 0
    if mistake == "a fully masked row takes only the live tiles":
        assert (d[:, :, 37] > 0).any() and not (np.delete(d, 37, axis=2) > 0).any()
