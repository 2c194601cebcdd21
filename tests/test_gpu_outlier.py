"""The outlier side path on the device: qt_filter_outlier_* / qt_spmm_csr_* (csrc/qt_outlier.hip) through the operators, the router
(quantized_training/outlier.py) and the C ABI.

filter_outlier: all four results bit for bit against the operator on CPU tensors, which tests/test_pt2e_cpu.py pins to the reference.
spmm_csr, exact tier: data = integers in [-127, 127] times 1 or 2, B = integers in [-127, 127] (or a 16-entry codebook of such), block
scales out of {0.5, 1, 2}.  Every product is a multiple of q = 0.5 and the test asserts sum |a||b| < 2^24 q for every row, so every
partial sum in ANY order is an fp32 number: the result must be the fp64 sum rounded once to the output dtype, bit for bit.
Tolerance tier: normal data, the standard bound of an fp32 accumulation of m terms, |y - y64| <= (m + 1) 2^-24 sum |a||b|, plus half a
bf16 ulp of y64 for a bf16 output; y64 is formed from the operand as the composite forms it (codebook, then the product with the block
scale rounded to the tensor's dtype)."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import quantized_training  # noqa: F401  (registers torch.ops.quantized_ops)
from kernel_launch import nv, stream  # noqa: F401

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="f32")]
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ops = torch.ops.quantized_ops


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu()


@pytest.fixture(autouse=True)
def stats():
    from quantized_training import outlier
    outlier.STATS.reset()
    return outlier.STATS


class Guard:
    """A device buffer between two bands of 0xFF."""
    PAD = 256

    def __init__(self, count, dtype):
        self.count, self.dtype = int(count), dtype
        self.nbytes = self.count * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.nbytes + 2 * self.PAD,), 0xFF, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.PAD

    def intact(self):
        return bool((self.raw[:self.PAD] == 0xFF).all()) and bool((self.raw[self.PAD + self.nbytes:] == 0xFF).all())

    def host(self):
        return self.raw[self.PAD:self.PAD + self.nbytes].cpu().view(self.dtype)


# ---- filter_outlier ----------------------------------------------------------------------------------------------------------------------
def assert_filter_equals_cpu(x, threshold, max_pct, stats, what=""):
    """-> the device results, after comparing all four with the CPU operator's bit for bit."""
    want = ops.filter_outlier(x, threshold, max_pct)
    got = ops.filter_outlier(x.cuda(), threshold, max_pct)
    torch.cuda.synchronize()
    assert (stats.native, stats.fallback) == (1, 0), what
    for name, a, b in zip(("inlier", "data", "indices", "indptr"), want, got):
        assert b.device.type == "cuda" and a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert torch.equal(bits(a), bits(b)), f"{what}: {name} differs in {int((bits(a) != bits(b)).sum())} of {a.numel()}"
    keep = min(int(want[3][-1]), want[1].numel())
    assert not bool(got[1][keep:].view(bits(got[1]).dtype).any()) and not bool(got[2][keep:].any()), f"{what}: padding"
    stats.reset()
    return got


def filter_input(rows, cols, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * 2
    x[0] = x[0] * 100 + 50                                       # a row of outliers only
    if rows > 1:
        x[rows // 2] *= 0.01                                     # a row without any
    return x.to(dtype)


# C = 257 / 513: one past a wave's single sweep of a row (64 lanes x 16 bytes: 256 fp32, 512 bf16); R = 4097: one past a scan chunk
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 3, 4097])
@pytest.mark.parametrize("cols", [1, 33, 96, 257, 513])
def test_filter_outlier_equals_the_cpu_operator(nv, stats, dtype, rows, cols):
    x = filter_input(rows, cols, dtype, rows * 1000 + cols)
    for threshold, max_pct in ((4.5, 0.05), (3.0, 0.05), (4.09, 0.5)):       # under the cap; truncated; a threshold bf16 rounds up
        assert_filter_equals_cpu(x, threshold, max_pct, stats, f"[{rows}, {cols}] threshold {threshold}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_outlier_on_a_3d_input(nv, stats, dtype):
    arr = np.load(os.path.join(G, "outlier.npz"))
    info = json.load(open(os.path.join(G, "outlier.json")))["op"]
    x = torch.from_numpy(arr["op__x"].view(np.float32).copy()).reshape(3, 5, 32).to(dtype)
    got = assert_filter_equals_cpu(x, info["threshold"], info["max_pct"], stats, "[3, 5, 32]")
    assert got[0].shape == (3, 5, 32) and got[3].numel() == 16
    if dtype == F32:
        assert int(got[3][-1]) == info["nnz"] and np.array_equal(got[2].cpu().numpy().astype(np.int64), arr["op__indices"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("planted,what", [(20, "nnz == max_nnz"), (23, "the cut inside a row"), (45, "rows behind the cut")])
def test_filter_outlier_at_the_cap(nv, stats, dtype, planted, what):
    x = torch.full((8, 50), 0.25)
    flat = x.view(-1)
    where = torch.arange(planted) * 7 + 91                        # rows 1 ..: entry 18 .. 22 share row 4 (columns 17 .. 45)
    flat[where] = torch.arange(planted).float() + 8
    got = assert_filter_equals_cpu(x.to(dtype), 4.0, 0.05, stats, what)
    assert got[1].numel() == 20 and int(got[3][-1]) == planted
    if planted == 23:
        assert int(got[3][4]) < 20 < int(got[3][5])


@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_outlier_with_max_nnz_zero(nv, stats, dtype):
    x = torch.tensor([[0.5, 9.0, -7.0, 0.0, 1.0], [8.0, 0.1, 0.2, -9.5, 0.3]]).to(dtype)
    got = assert_filter_equals_cpu(x, 4.0, 0.05, stats, "max_nnz == 0")
    assert got[1].numel() == 0 and got[2].numel() == 0 and got[3].tolist() == [0, 2, 4]


SPECIALS = [float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 1e-40, -1e-40, 2.0 ** -133, 3.0, -3.0, 3.5, -1e30, 65504.0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("threshold", [0.0, -1.0, 3.0, float("inf")])
def test_filter_outlier_zeros_nan_inf_subnormals(nv, stats, dtype, threshold):
    """Threshold 0 and a negative one on +-0.0 (no zero is emitted, -0.0 survives only where it is no outlier); NaN is never an
    outlier and keeps its bits; an inf at the threshold stays; subnormals are non-zero."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 40, generator=g)
    where = torch.randperm(200, generator=g)[:3 * len(SPECIALS)]
    x.view(-1)[where] = torch.tensor(SPECIALS * 3)
    x.view(torch.int32).view(-1)[where[0]] = 0x7FC12345           # a NaN with a payload
    if dtype == BF16:                                             # truncation keeps the specials what they are
        x = x.view(torch.int32).bitwise_right_shift(16).to(torch.int16).view(BF16)
    got = assert_filter_equals_cpu(x, threshold, 1.0, stats, f"threshold {threshold}")
    assert not bool((got[1][:int(got[3][-1])] == 0).any())
    assert int(got[0].isnan().sum()) == int(x.isnan().sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_outlier_makes_a_strided_input_contiguous(nv, stats, dtype):
    x = filter_input(37, 21, dtype, 77).t()
    assert not x.is_contiguous()
    assert_filter_equals_cpu(x, 3.0, 0.2, stats, "transposed view")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,offset,out_offset", [(5, 33, 0, 0), (4, 96, 3, 3), (3, 513, 1, 0), (3, 96, 0, 2)])
def test_filter_outlier_keeps_inside_its_buffers(nv, dtype, rows, cols, offset, out_offset):
    """The C entry point into guarded buffers (the input `offset`, the inlier `out_offset` elements off a 16-byte boundary): status 0,
    the bands of 0xFF around all four results intact, results equal to the CPU operator's."""
    x = filter_input(rows, cols, dtype, 3)
    want = ops.filter_outlier(x, 3.0, 0.05)
    max_nnz = want[1].numel()
    src = torch.zeros(x.numel() + 16, dtype=dtype, device="cuda")
    src[offset:offset + x.numel()] = x.reshape(-1).cuda()
    es = x.element_size()
    inl, data, idx, ptr = Guard(x.numel() + out_offset, dtype), Guard(max_nnz, dtype), Guard(max_nnz, torch.int32), Guard(rows + 1, torch.int32)
    fn = nv.lib().qt_filter_outlier_bf16 if dtype == BF16 else nv.lib().qt_filter_outlier_f32
    rc = fn(src.data_ptr() + offset * es, inl.ptr + out_offset * es, data.ptr, idx.ptr, ptr.ptr, rows, cols, 3.0, max_nnz, stream())
    torch.cuda.synchronize()
    assert rc == 0
    for g in (inl, data, idx, ptr):
        assert g.intact()
    assert bool((inl.raw[Guard.PAD:Guard.PAD + out_offset * es] == 0xFF).all())
    assert torch.equal(bits(inl.host()[out_offset:]), bits(want[0].reshape(-1)))
    assert torch.equal(bits(data.host()), bits(want[1])) and torch.equal(idx.host(), want[2]) and torch.equal(ptr.host(), want[3])


def test_filter_outlier_still_warns_about_truncation(nv, stats, caplog):
    x = (torch.randn(16, 64, generator=torch.Generator().manual_seed(9)) * 2).cuda()
    with caplog.at_level(logging.WARNING, logger="quantized_training.decomposed"):
        ops.filter_outlier(x, 20.0, 0.05)
        assert not [r for r in caplog.records if "truncating" in r.getMessage()]
        _, data, _, ptr = ops.filter_outlier(x, 1.0, 0.05)
    assert stats.native == 2 and int(ptr[-1]) > data.numel()
    msgs = [r.getMessage() for r in caplog.records if "truncating" in r.getMessage()]
    assert msgs == [f"Number of non-zero elements {int(ptr[-1])} exceeds max_nnz {data.numel()}, truncating."]


# ---- spmm_csr ----------------------------------------------------------------------------------------------------------------------------
def expand64(scale, shape, bs):
    s = scale.double()
    for dim in range(2):
        if s.shape[dim] != shape[dim]:
            s = s.repeat_interleave(bs, dim)
    return s[:shape[0], :shape[1]]


def operand_in_dtype(B, scale, code, bs):
    """Bd as the composite forms it on the host, in the tensor's dtype, [stored layout]."""
    if code is not None:
        B = code[B.to(torch.long)]
    if scale is not None:
        s = scale
        for dim in range(2):
            if s.shape[dim] != B.shape[dim]:
                s = s.repeat_interleave(bs, dim)
        B = B * s[:B.shape[0], :B.shape[1]]
    return B


def spmm64(data, idx, ptr, Bd_nk, cap=None):
    """fp64 oracle on the stored entries -> (Y [M, N], sum |a||b| [M, N], entries per row [M])"""
    cap = data.numel() if cap is None else cap
    d, Bd = data.double().numpy(), Bd_nk.double().numpy()
    M = ptr.numel() - 1
    Y, A, m = np.zeros((M, Bd.shape[0])), np.zeros((M, Bd.shape[0])), np.zeros(M)
    for r in range(M):
        s, e = min(int(ptr[r]), cap), min(int(ptr[r + 1]), cap)
        cols = idx[s:e].numpy()
        Y[r] = Bd[:, cols] @ d[s:e]
        A[r] = np.abs(Bd[:, cols]) @ np.abs(d[s:e])
        m[r] = e - s
    return torch.from_numpy(Y), torch.from_numpy(A), torch.from_numpy(m)


def csr(counts, K, values, seed):
    """Rows of `counts[r]` entries with sorted distinct columns (`values(n, g)` makes the data)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.cat([torch.randperm(K, generator=g)[:c].sort().values for c in counts] + [torch.zeros(0, dtype=torch.long)]).to(torch.int32)
    ptr = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32)
    return values(int(idx.numel()), g), idx, ptr


COUNTS = [0, 1, 300, 5, 0, 0, 64, 65, 17, 1]                      # rows without entries, with one, with more than a summation group of 16, a wave of lanes


def exact_problem(N, K, dtype, scaled, coded, transposed, counts=COUNTS, seed=0, mag=127):
    def values(n, g):
        return (torch.randint(-mag, mag + 1, (n,), generator=g).float() * (1 + torch.randint(0, 2, (n,), generator=g))).to(dtype)
    data, idx, ptr = csr(counts, K, values, seed + N)
    g = torch.Generator().manual_seed(seed + 17 * N + K)
    code = None
    if coded:
        code = torch.randint(-mag, mag + 1, (16,), generator=g).to(dtype)
        B = torch.randint(0, 16, (N, K), generator=g).to(dtype)
    else:
        B = torch.randint(-mag, mag + 1, (N, K), generator=g).to(dtype)
    scale = (2.0 ** torch.randint(-1, 2, (N, (K + 31) // 32), generator=g).float()).to(dtype) if scaled else None
    Bd = operand_in_dtype(B, scale, code, 32)
    if transposed:
        B, scale = B.t().contiguous(), scale.t().contiguous() if scale is not None else None
    y64, a64, _ = spmm64(data, idx, ptr, Bd)
    assert float(a64.max()) / 0.5 < 2 ** 24                        # every partial sum in any order is an fp32 number
    return dict(data=data, idx=idx, ptr=ptr, B=B, scale=scale, code=code, bs=32 if scaled else None, transposed=transposed), y64


def run_op(p):
    f = lambda t: None if t is None else t.cuda()
    return ops.spmm_csr(f(p["data"]), f(p["idx"]), f(p["ptr"]), f(p["B"]), f(p["scale"]), f(p["code"]), p["bs"], p["transposed"])


def run_c(nv, p, dtype, cap=None):
    """The C entry point into a guarded output -> Y on the host."""
    f = lambda t: None if t is None else t.cuda()
    d = {k: f(p[k]) for k in ("data", "idx", "ptr", "B", "scale", "code")}
    M = p["ptr"].numel() - 1
    N, K = (p["B"].shape[1], p["B"].shape[0]) if p["transposed"] else p["B"].shape
    cap = p["data"].numel() if cap is None else cap
    sv = (0, 0, 0, 0)
    if p["scale"] is not None:
        sv = tuple(p["scale"].shape) + tuple(1 if s == b else p["bs"] for s, b in zip(p["scale"].shape, p["B"].shape))
    y = Guard(M * N, dtype)
    fn = nv.lib().qt_spmm_csr_bf16 if dtype == BF16 else nv.lib().qt_spmm_csr_f32
    rc = fn(d["data"].data_ptr(), d["idx"].data_ptr(), d["ptr"].data_ptr(), cap, M, d["B"].data_ptr(), N, K, int(p["transposed"]),
            d["scale"].data_ptr() if d["scale"] is not None else None, *sv, d["code"].data_ptr() if d["code"] is not None else None,
            0 if d["code"] is None else d["code"].numel(), y.ptr, stream())
    torch.cuda.synchronize()
    assert rc == 0 and y.intact()
    return y.host().reshape(M, N)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("transposed", [False, True], ids=["NK", "KN"])
@pytest.mark.parametrize("variant", ["plain", "scaled", "codebook", "codebook+scaled"])
@pytest.mark.parametrize("N", [1, 40, 257])
def test_spmm_csr_exact_tier(nv, stats, dtype, transposed, variant, N):
    p, y64 = exact_problem(N, 330, dtype, "scaled" in variant, "codebook" in variant, transposed)       # K = 330: a last block of 10
    want = y64.float().to(dtype)                                   # (an fp32 number) rounded once
    y = run_op(p)
    assert (stats.native, stats.fallback) == (1, 0) and y.dtype == dtype and y.shape == (len(COUNTS), N)
    bad = bits(y) != bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} differ, largest {float((y.cpu().double() - y64).abs().max())}"
    assert torch.equal(bits(run_c(nv, p, dtype)), bits(want))      # output guards
    assert not bool(y[0].any()) and not bool(y[4].any())            # rows without entries are written, as zeros


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("transposed", [False, True], ids=["NK", "KN"])
def test_spmm_csr_many_rows_and_an_empty_csr(nv, stats, dtype, transposed):
    """2500 rows (more than one sweep of a workgroup's threads, and rows split over workgroups when the features fill few tiles), and
    a CSR without any entry."""
    counts = [(r * 7) % 5 for r in range(2500)]
    for N in (3, 40):
        p, y64 = exact_problem(N, 96, dtype, True, False, transposed, counts=counts, seed=4)
        assert torch.equal(bits(run_op(p)), bits(y64.float().to(dtype)))
    p, _ = exact_problem(40, 96, dtype, True, False, transposed, counts=[0] * 7)
    p["data"], p["idx"] = torch.ones(12, dtype=dtype), torch.zeros(12, dtype=torch.int32)
    y = run_op(p)
    assert y.shape == (7, 40) and not bool(y.any()) and stats.native == 3


def normal_problem(N, K, dtype, transposed, seed=1):
    counts = [0, 1, 2, 300, 41, 64, 65, 128, 7, 200, 33, 90]
    data, idx, ptr = csr(counts, K, lambda n, g: (torch.randn(n, generator=g) * 6).to(dtype), seed)
    g = torch.Generator().manual_seed(seed + 100)
    B = torch.randn(N, K, generator=g).to(dtype)
    scale = (torch.rand(N, (K + 31) // 32, generator=g) + 0.25).to(dtype)
    Bd = operand_in_dtype(B, scale, None, 32)
    if transposed:
        B, scale = B.t().contiguous(), scale.t().contiguous()
    return dict(data=data, idx=idx, ptr=ptr, B=B, scale=scale, code=None, bs=32, transposed=transposed), spmm64(data, idx, ptr, Bd)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("transposed", [False, True], ids=["NK", "KN"])
def test_spmm_csr_tolerance_tier_and_the_composite(nv, stats, dtype, transposed, monkeypatch):
    p, (y64, a64, m) = normal_problem(257, 330, dtype, transposed)
    y = run_op(p)
    assert stats.native == 1
    err = (y.cpu().double() - y64).abs()
    bound = (m[:, None] + 1) * 2.0 ** -24 * a64
    if dtype == BF16:
        bound = bound + 2.0 ** (torch.floor(torch.log2(y64.abs().clamp_min(1e-300))) - 8)       # half a bf16 ulp of y64
    print(f"\n[spmm_csr {dtype} transposed={transposed}] largest error {float(err.max()):.3e}, largest error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements outside the bound, worst ratio {float((err / bound).max())}"
    assert torch.equal(bits(run_op(p)), bits(y))                    # deterministic
    monkeypatch.setenv("QT_MX_GEMM", "0")
    composite = run_op(p)
    assert stats.fallback == 1
    cerr = (composite.cpu().double() - y64).abs()
    print(f"[spmm_csr {dtype} transposed={transposed}] composite's largest error {float(cerr.max()):.3e}")
    assert float(err.max()) <= float(cerr.max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("transposed", [False, True], ids=["NK", "KN"])
def test_spmm_csr_truncated_csr_is_safe(nv, dtype, transposed):
    """indptr counts 493 entries, the arrays hold 200: data / indices are views into larger allocations whose tails hold NaN and
    in-range but wrong indices.  The C entry point multiplies the stored entries only."""
    p, _ = exact_problem(40, 330, dtype, True, False, transposed)
    cap = 200                                                      # inside row 2
    full_d, full_i = p["data"].clone(), p["idx"].clone()
    full_d[cap:] = float("nan")
    full_i[cap:] = (full_i[cap:] * 13 + 5) % 330
    Bd = operand_in_dtype(p["B"].t() if transposed else p["B"], p["scale"].t() if transposed else p["scale"], None, 32)
    y64, _, _ = spmm64(p["data"], p["idx"], p["ptr"], Bd, cap=cap)
    q = dict(p, data=full_d, idx=full_i)
    y = run_c(nv, q, dtype, cap=cap)
    assert not bool(y.isnan().any()) and torch.equal(bits(y), bits(y64.float().to(dtype)))
    assert not bool(y[3:].any())                                    # rows wholly behind the cut


def test_spmm_csr_still_raises_on_a_truncated_csr(nv, stats):
    x = filter_input(16, 64, F32, 9).cuda()
    _, data, idx, ptr = ops.filter_outlier(x, 1.0, 0.05)
    assert int(ptr[-1]) > data.numel()
    with pytest.raises(IndexError):
        ops.spmm_csr(data, idx, ptr, torch.ones(8, 64, device="cuda"))
    assert stats.native == 2


# ---- stream capture ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_pair_is_captured_and_replayed(nv, stats, dtype):
    """filter_outlier -> spmm_csr in a captured graph, replayed on fresh contents -- one of them truncates -- against the eager calls
    (the truncated product against the C entry point, which eager calls refuse with IndexError)."""
    g = torch.Generator().manual_seed(2)
    W = torch.randint(-8, 9, (40, 96), generator=g).to(dtype).cuda()
    S = (2.0 ** torch.randint(-1, 2, (40, 3), generator=g).float()).to(dtype).cuda()
    contents = [filter_input(64, 96, dtype, s) for s in (21, 22)] + [filter_input(64, 96, dtype, 23) * 3]
    static = contents[0].cuda().clone()

    def pair():
        inl, data, idx, ptr = ops.filter_outlier(static, 4.5, 0.05)
        return inl, data, idx, ptr, ops.spmm_csr(data, idx, ptr, W, S, None, 32)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    stats.reset()
    with torch.cuda.graph(graph):
        outs = pair()
    assert (stats.native, stats.fallback) == (2, 0)
    truncated = 0
    for x in contents:
        static.copy_(x.cuda())
        graph.replay()
        torch.cuda.synchronize()
        got = [bits(t) for t in outs]
        eager = ops.filter_outlier(x.cuda(), 4.5, 0.05)
        for a, b in zip(got[:4], eager):
            assert torch.equal(a, bits(b))
        if int(eager[3][-1]) > eager[1].numel():
            truncated += 1
            p = dict(data=eager[1], idx=eager[2], ptr=eager[3], B=W, scale=S, code=None, bs=32, transposed=False)
            y = run_c(nv, p, dtype)
        else:
            y = ops.spmm_csr(eager[1], eager[2], eager[3], W, S, None, 32)
        assert torch.equal(got[4], bits(y))
    assert truncated == 1


# ---- the converted model -----------------------------------------------------------------------------------------------------------------
def converted_two_linear(device):
    from quantized_training import quantize_pt2e as qp
    info = json.load(open(os.path.join(G, "outlier.json")))["model"]
    arr = np.load(os.path.join(G, "outlier.npz"))

    class Two(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1 = torch.nn.Linear(64, 128)
            self.fc2 = torch.nn.Linear(128, 64)

        def forward(self, x):
            return self.fc2(torch.relu(self.fc1(x)))

    m = Two().eval()
    r = np.random.default_rng(3)
    with torch.no_grad():
        for n, p in sorted(m.named_parameters()):
            p.copy_(torch.from_numpy((r.standard_normal(tuple(p.shape)) * 0.1).astype(np.float32)))
    m = m.to(device)
    x0, x1 = (torch.from_numpy(arr[k].view(np.float32).copy()).reshape(16, 64).to(device) for k in ("x0", "x1"))
    gm = qp.prepare_pt2e(m, qp.get_default_quantizer(**info["kw"]), (x0,))
    with torch.no_grad():
        gm(x0)
        gm(x1)
    return qp.convert_pt2e(gm), x1


def test_converted_model_runs_the_kernels_and_replays(nv, stats):
    gc_cpu, x_cpu = converted_two_linear("cpu")
    gc, x = converted_two_linear("cuda")
    with torch.no_grad():
        want = gc_cpu(x_cpu)
        stats.reset()
        y = gc(x)
    assert (stats.native, stats.fallback) == (4, 0)                 # filter_outlier and spmm_csr, per layer
    assert float((want - y.cpu()).abs().max()) <= 1e-5 * float(want.abs().max())
    static = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        gc(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = gc(static)
    for scale in (1.0, 0.5):
        static.copy_(x * scale)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            assert torch.equal(bits(out), bits(gc(x * scale)))


# ---- fallbacks ---------------------------------------------------------------------------------------------------------------------------
def composite_only(monkeypatch):
    from quantized_training import outlier
    monkeypatch.setattr(outlier, "filter_outlier_or_none", lambda *a, **k: None)
    monkeypatch.setattr(outlier, "spmm_csr_or_none", lambda *a, **k: None)


@pytest.mark.parametrize("case", ["QT_MX_GEMM=0", "fp16", "int64 indices", "65536-entry codebook"])
def test_fallbacks_run_the_composite(nv, stats, monkeypatch, case):
    """Exact-tier operands, so that the composite's sum does not depend on the order of its atomics and equality is bit for bit."""
    dtype = torch.float16 if case == "fp16" else F32
    p, y64 = exact_problem(40, 96, F32, True, False, False, counts=[0, 3, 9, 1, 5], mag=3)          # |sums| <= 324: exact in fp16 too
    x = filter_input(9, 40, F32, 1).to(dtype).cuda()
    if case == "65536-entry codebook":
        p["code"] = (torch.arange(65536) % 255 - 127).float()
        p["B"] = torch.randint(0, 65536, (40, 96), generator=torch.Generator().manual_seed(1)).float()
    if case == "int64 indices":
        p["idx"] = p["idx"].long()
    for k in ("data", "B", "scale", "code"):
        p[k] = None if p[k] is None else p[k].to(dtype)
    if case == "QT_MX_GEMM=0":
        monkeypatch.setenv("QT_MX_GEMM", "0")
    y = run_op(p)
    assert (stats.native, stats.fallback) == (0, 1)
    filtered = None
    if case in ("QT_MX_GEMM=0", "fp16"):
        filtered = ops.filter_outlier(x, 3.0, 0.05)
        assert (stats.native, stats.fallback) == (0, 2)
    composite_only(monkeypatch)
    stats.reset()
    assert torch.equal(bits(run_op(p)), bits(y))
    if filtered is not None:
        for a, b in zip(filtered, ops.filter_outlier(x, 3.0, 0.05)):
            assert torch.equal(bits(a), bits(b))
    assert (stats.native, stats.fallback) == (0, 0)
