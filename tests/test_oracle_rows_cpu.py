"""The row-reduction oracles (oracle/qt_oracle.py: rmsnorm, layernorm, layernorm_backward, softmax_backward, softmax_interval,
causal_lm_nll) without a GPU.

(1) Each restatement is pinned, on N(0, sigma) rows, to the torch CPU chain it restates: every torch result lies in [lo, hi] and every
    decided element is bit-equal.
(2) For every case tests/test_gpu_row_kernels.py launches (oracle/row_cases.py), the conditions those tests rely on hold from the oracle
    alone: at least 95 % of the finite elements of the well-conditioned rows are decided, and every named degenerate row has its
    closed-form value.  Rows exempt from the share (checked by the interval only) are listed by name in row_cases.LN_ILL_CONDITIONED
    (constant rows, |mean| / std >= 32) and row_cases.SOFTMAX_EXEMPT (probabilities in the fp32 subnormal range); rows that are NaN
    throughout have no finite element to count.
"""
import math

import numpy as np
import pytest
import torch

from oracle import qt_oracle as o
from oracle import row_cases as rc

SHARE = 0.95


def t_bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def bits_of(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def rand_bits(shape, sigma, seed, offset=0.0):
    g = np.random.default_rng(seed)
    return o.f32_to_bf16((g.standard_normal(shape) * sigma + offset).astype(np.float32))


def assert_inside(iv, got_bits, what):
    d = iv.distance(got_bits)
    assert int(d.max()) == 0, f"{what}: {iv.report(got_bits)}"
    dec = iv.decided
    assert np.array_equal(o.bf16_order(np.asarray(got_bits)[dec]), o.bf16_order(iv.lo[dec])), what


def share_of(iv, rows_mask):
    return iv.rows(rows_mask).decided_share() if rows_mask.any() else 1.0


# ---- (1) pinned to torch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,sigma,eps", [(64, 1.0, 1e-6), (1000, 7.0, 1e-5), (4096, 0.02, 1e-6)])
@pytest.mark.parametrize("residual", [False, True])
def test_rmsnorm_restates_llama_rmsnorm(cols, sigma, eps, residual):
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    x, r, w = rand_bits((6, cols), sigma, 1), rand_bits((6, cols), sigma, 2), rand_bits((cols,), 0.1, 3, 1.0)
    norm = LlamaRMSNorm(cols, eps=eps).bfloat16()
    with torch.no_grad():
        norm.weight.copy_(t_bf16(w))
        s = t_bf16(x) + t_bf16(r) if residual else t_bf16(x)
        want = norm(s)
    iv, sum_bits = o.rmsnorm(x, w, eps, r if residual else None)
    if residual:
        assert np.array_equal(sum_bits, bits_of(s))
    assert_inside(iv, bits_of(want), "rmsnorm")
    assert iv.decided_share() >= SHARE


@pytest.mark.parametrize("cols,sigma,offset,eps", [(64, 1.0, 0.0, 1e-5), (1000, 3.0, 0.5, 1e-12), (4096, 0.5, -0.1, 1e-5)])
@pytest.mark.parametrize("residual", [False, True])
def test_layernorm_restates_layer_norm_on_bf16(cols, sigma, offset, eps, residual):
    x, r = rand_bits((6, cols), sigma, 4, offset), rand_bits((6, cols), sigma, 5)
    w, b = rand_bits((cols,), 0.1, 6, 1.0), rand_bits((cols,), 0.1, 7)
    s = t_bf16(x) + t_bf16(r) if residual else t_bf16(x)
    want, mean, rstd = torch.native_layer_norm(s, [cols], t_bf16(w), t_bf16(b), eps)
    res = o.layernorm(x, w, b, eps, r if residual else None)
    if residual:
        assert np.array_equal(res.sum_bits, bits_of(s))
    assert_inside(res.y, bits_of(want), "layernorm")
    assert res.y.decided_share() >= SHARE
    mean, rstd = mean.double().numpy().reshape(-1), rstd.double().numpy().reshape(-1)
    # (torch returns the statistics of a bf16 tensor rounded to bf16)
    assert np.all(np.abs(mean - res.mean) <= res.rho_mean + 2.0 ** -8 * np.abs(res.mean))
    assert np.all((rstd >= res.rstd_lo * (1 - 2.0 ** -8)) & (rstd <= res.rstd_hi * (1 + 2.0 ** -8)))


@pytest.mark.parametrize("rows,cols,sigma", [(5, 64, 1.0), (33, 1000, 2.0), (9, 1024, 1e-3)])
def test_layernorm_backward_restates_native_layer_norm_backward(rows, cols, sigma):
    x, dy = rand_bits((rows, cols), 2.0, 8, 0.3), rand_bits((rows, cols), sigma, 9)
    w, b = rand_bits((cols,), 0.1, 10, 1.0), rand_bits((cols,), 0.1, 11)
    xf = t_bf16(x).float()
    mean = xf.mean(-1)
    rstd = (xf.var(-1, unbiased=False) + 1e-5).rsqrt()
    # dx: the bf16 call (fp32 parameters: the CPU kernel takes fp32 statistics next to bf16 rows only that way; their values are the bf16
    # ones).  dgamma / dbeta: the same operator on the fp32 images of the same tensors -- the chain restated is fp32 sums of fp32 terms,
    # and the CPU kernel's bf16 path keeps its per-thread partial sums in bf16, 2^-9 relative each, which no fp32 radius holds
    stats = (mean.view(rows, 1), rstd.view(rows, 1), t_bf16(w).float(), t_bf16(b).float(), [True, True, True])
    gx = torch.ops.aten.native_layer_norm_backward(t_bf16(dy), t_bf16(x), [cols], *stats)[0]
    _, gw, gb = torch.ops.aten.native_layer_norm_backward(t_bf16(dy).float(), xf, [cols], *stats)
    dx, dgamma, dbeta = o.layernorm_backward(dy, x, w, mean.numpy(), rstd.numpy())
    assert_inside(dx, bits_of(gx), "dx")
    assert np.all(np.abs(gw.double().numpy() - dgamma.v) <= dgamma.rho) and np.all(np.abs(gb.double().numpy() - dbeta.v) <= dbeta.rho)
    assert_inside(dgamma, bits_of(gw.bfloat16()), "dgamma")
    assert_inside(dbeta, bits_of(gb.bfloat16()), "dbeta")
    assert dx.decided_share() >= SHARE


@pytest.mark.parametrize("cols,dp_std", [(64, 1.0), (1000, 1e-4), (2048, 1.0)])
def test_softmax_backward_restates_softmax_backward_data_times_scaling(cols, dp_std):
    scaling = 0.125
    sc = rand_bits((7, cols), 3 / scaling, 12)
    p = o.softmax_fq(sc, None, scaling, None)[0]
    dp = rand_bits((7, cols), dp_std, 13)
    want = torch.ops.aten._softmax_backward_data(t_bf16(dp), t_bf16(p), -1, torch.bfloat16) * scaling
    iv = o.softmax_backward(dp, p, scaling)
    assert_inside(iv, bits_of(want), "softmax backward")
    assert iv.decided_share() >= SHARE


@pytest.mark.parametrize("cols,sigma", [(64, 3.0), (1000, 40.0), (4096, 3.0)])
def test_softmax_interval_holds_torch_softmax_and_the_oracle_s_own_pattern(cols, sigma):
    scaling = 0.125
    sc = rand_bits((7, cols), sigma, 14)
    mask = np.zeros((7, cols), np.uint16)
    mask[::2, cols - cols // 3:] = rc.BF16_MIN
    t = (t_bf16(sc) * scaling) + t_bf16(mask)
    want = torch.softmax(t, -1, dtype=torch.float32).bfloat16()
    p_bits, pq_bits, iv = o.softmax_fq(sc, mask, scaling, o.get_quantization_map("e4m3"), with_interval=True)
    plain = o.softmax_fq(sc, mask, scaling, o.get_quantization_map("e4m3"))
    assert len(plain) == 2 and np.array_equal(plain[0], p_bits) and np.array_equal(plain[1], pq_bits)      # what it returned before
    assert_inside(iv, bits_of(want), "softmax")
    assert_inside(iv, p_bits, "softmax_fq")
    assert iv.decided_share() >= SHARE


@pytest.mark.parametrize("B,S,V", [(2, 5, 7), (1, 9, 1003), (2, 4, 2056)])
def test_causal_lm_nll_restates_cross_entropy_on_float_logits(B, S, V):
    bits = rand_bits((B, S, V), 4.0, 15)
    g = np.random.default_rng(16)
    labels = g.integers(0, V, (B, S))
    labels[0, 1] = -100
    loss, rho, scored, mean, rho_mean = o.causal_lm_nll(bits, labels)
    logits = t_bf16(bits).float()
    lab = torch.from_numpy(labels)
    per = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), lab[:, 1:].reshape(-1), ignore_index=-100, reduction="none")
    per = per.view(B, S - 1).double().numpy()
    assert not scored[:, -1].any() and not scored[0, 0]
    sc = scored[:, :-1]
    assert np.all(np.abs(per[sc] - loss[:, :-1][sc]) <= rho[:, :-1][sc])
    want = float(torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), lab[:, 1:].reshape(-1), ignore_index=-100))
    assert abs(want - mean) <= rho_mean
    assert rho_mean <= 1e-4 * max(1.0, mean)                    # the radius is not vacuous


# ---- (2) what the GPU cases rely on -----------------------------------------------------------------------------------------------------
def _row(names, name):
    return [i for i, n in enumerate(names) if n == name]


@pytest.mark.parametrize("cols", rc.RMS_COLS)
@pytest.mark.parametrize("residual", [False, True])
def test_rmsnorm_cases(cols, residual):
    c = rc.norm_case("rms", cols, residual)
    iv, _ = o.rmsnorm(c["x"], c["w"], 1e-6, c["res"])
    wc = rc.well_conditioned(c["names"])
    assert share_of(iv, wc) >= SHARE
    for nm in ("zero", "overflow"):                               # y == +-0, decided
        r = iv.rows(_row(c["names"], nm))
        assert np.all(o.bf16_order(r.lo) == 0) and np.all(o.bf16_order(r.hi) == 0), nm
    # the x1.37 row sees an error in r: r off by 2^-12 relative either way (the mean square taken over cols - 8 at the longest row is
    # that far off) puts elements outside the interval
    i = _row(c["names"], "n01_x1.37")
    s = o.bf16_to_f32(c["x"][i] if c["res"] is None else o.bf16_add(c["x"][i], c["res"][i])).astype(np.float64)
    for off in (1 + 2.0 ** -12, 1 - 2.0 ** -12):
        h_off = o.f32_to_bf16((s * (off / np.sqrt((s * s).mean() + 1e-6))).astype(np.float32))
        y_off = o.f32_to_bf16(o.bf16_to_f32(c["w"]) * o.bf16_to_f32(h_off))
        assert int((iv.rows(i).distance(y_off) > 0).sum()) >= cols // 64
    r = iv.rows(_row(c["names"], "one_nan"))
    assert r.nan.all()
    r = iv.rows(_row(c["names"], "one_inf"))                      # r = 0: zeros, NaN at the inf itself
    assert r.nan.sum() == 1 and r.nan[0, cols - 1] and np.all(o.bf16_order(r.lo)[~r.nan] == 0) and np.all(o.bf16_order(r.hi)[~r.nan] == 0)


@pytest.mark.parametrize("cols", rc.LN_COLS + rc.LN_CONST_COLS)
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("eps", rc.LN_EPS)
def test_layernorm_cases(cols, residual, eps):
    c = rc.norm_case("ln", cols, residual)
    res = o.layernorm(c["x"], c["w"], c["b"], eps, c["res"])
    assert share_of(res.y, rc.well_conditioned(c["names"])) >= SHARE
    bias = np.broadcast_to(c["b"], (1, cols))
    for nm in ("zero", "overflow"):                               # y == bias, decided
        r = res.y.rows(_row(c["names"], nm))
        assert np.array_equal(r.lo, bias) and np.array_equal(r.hi, bias), nm
    for nm in ("const1", "const3", "const5.5"):                   # the exact answer is the bias: inside the interval (not decided)
        i = _row(c["names"], nm)
        s = o.bf16_to_f32(c["x"][i] if c["res"] is None else o.bf16_add(c["x"][i], c["res"][i]))
        assert np.all(s == float(nm[5:]))
        assert int(res.y.rows(i).distance(bias).max()) == 0, nm
    for nm in ("one_nan", "one_inf"):
        assert res.y.rows(_row(c["names"], nm)).nan.all()
    r = _row(c["names"], "offset64")[0]
    assert abs(res.mean[r]) / math.sqrt(1 / res.rstd[r] ** 2) >= 32


@pytest.mark.parametrize("cols", rc.TRAIN_COLS)
@pytest.mark.parametrize("rows", rc.TRAIN_ROWS)
def test_layernorm_train_cases(rows, cols):
    c = rc.train_case(rows, cols)
    res = o.layernorm(c["x"], c["w"], c["b"], 1e-5)
    assert share_of(res.y, rc.well_conditioned(c["names"])) >= SHARE
    assert not res.y.nan.any()
    # the backward from the oracle's own statistics rounded to fp32 (the GPU test takes the kernel's)
    dx, dgamma, dbeta = o.layernorm_backward(c["dy"], c["x"], c["w"], res.mean.astype(np.float32), res.rstd.astype(np.float32))
    assert dx.decided_share() >= SHARE
    assert not dx.nan.any() and not dgamma.nan.any() and not dbeta.nan.any()


@pytest.mark.parametrize("cols", rc.SOFTMAX_COLS)
@pytest.mark.parametrize("scaling", rc.SOFTMAX_SCALINGS)
@pytest.mark.parametrize("mask_kind", rc.SOFTMAX_MASKS)
def test_softmax_cases(cols, scaling, mask_kind):
    c = rc.softmax_case(cols, scaling, mask_kind)
    iv = o.softmax_interval(c["scores"], c["mask"], scaling)
    flat = o.RowInterval(iv.v.reshape(-1, cols), iv.rho.reshape(-1, cols), iv.lo.reshape(-1, cols), iv.hi.reshape(-1, cols))
    names = c["names"]
    assert share_of(flat, rc.softmax_share_rows(names)) >= SHARE
    one = 0x3F80
    for i, nm in enumerate(names):
        lo, hi = flat.lo[i], flat.hi[i]
        q = i % c["Q"]
        tail_masked = mask_kind == "per_bq" and not nm.startswith("mask_") and q % 2
        if nm == "all_equal" and mask_kind == "none" and cols & (cols - 1) == 0:
            want = o.f32_to_bf16(np.float32(1.0 / cols))          # uniform, C a power of two: exactly 1 / C
            assert np.all(lo == want) and np.all(hi == want)
        if nm == "mask_fully_masked" and cols & (cols - 1) == 0:
            want = o.f32_to_bf16(np.float32(1.0 / cols))          # a fully masked row is uniform over ALL columns
            assert np.all(lo == want) and np.all(hi == want)
        if nm in ("mask_first_live", "mask_last_live"):           # one-hot: exactly 1 and zeros elsewhere
            k = 0 if nm == "mask_first_live" else cols - 1
            assert lo[k] == one and hi[k] == one
            assert np.all(np.delete(lo, k) == 0) and np.all(np.delete(hi, k) == 0)
        if nm == "dominant_dead" and not tail_masked:
            k = cols // 3
            assert lo[k] == one and hi[k] == one and np.all(np.delete(lo, k) == 0) and np.all(np.delete(hi, k) == 0)
        if nm in ("one_nan", "mask_neginf_row"):
            assert flat.nan[i].all()
        elif nm == "mask_neginf_part":
            assert not flat.nan[i].any() and np.all(lo[cols // 2:] == 0) and np.all(hi[cols // 2:] == 0)
        else:
            assert not flat.nan[i].any()


@pytest.mark.parametrize("cols", rc.SOFTMAX_BWD_COLS)
@pytest.mark.parametrize("dp_std", [1e-4, 1.0])
def test_softmax_backward_cases(cols, dp_std):
    c = rc.softmax_bwd_case(cols, dp_std)
    iv = o.softmax_backward(c["dp"], c["p"], c["scaling"])
    names = np.array(c["names"])
    assert share_of(iv, names == "softmax") >= SHARE
    assert share_of(iv, names == "uniform") >= SHARE
    hot = iv.rows(names == "one_hot")                             # ds == 0 exactly
    assert np.all(o.bf16_order(hot.lo) == 0) and np.all(o.bf16_order(hot.hi) == 0)


@pytest.mark.parametrize("shape", rc.LOSS_SHAPES)
@pytest.mark.parametrize("regime", rc.LOSS_REGIMES)
def test_loss_cases(shape, regime):
    c = rc.loss_case(shape, regime)
    if c is None:
        assert regime == "first8_neginf" and shape[2] <= 8
        return
    B, S, V, stride = shape
    loss, rho, scored, mean, rho_mean = o.causal_lm_nll(c["logits"][..., :V], c["labels"])
    assert not scored[:, -1].any()
    if regime == "all_ignored" or S == 1:
        assert not scored.any() and math.isnan(mean)
        return
    assert scored.any()
    if regime == "one_posinf":
        assert np.isnan(loss[scored]).all() and math.isnan(mean)
        return
    assert np.all(np.isfinite(loss[scored])) and np.all(rho[scored] <= 2.0 ** -12)
    if regime == "label_on_dominant":
        assert np.all(loss[scored] == 0.0)
    if regime == "label_off_dominant":
        assert np.all(np.abs(loss[scored] - 160.0) <= rho[scored])
    if regime == "all_equal":
        assert np.all(np.abs(loss[scored] - math.log(V)) <= 1e-12)
