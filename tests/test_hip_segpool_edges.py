"""nrms_segment_pool_fwd / _bwd (csrc/segpool.hip) where its kernels change behaviour, against the float64 statement of
tests/segpool_ref.py: segments longer than a wavefront (the 64-lane strides make further turns, the four-at-a-time row sum meets
every tail), rows whose sorted runs sit in each situation of the span path, a capacity beyond the lists' real length, the widths
at which the per-lane column ownership and seg_logit's stride end, the row counts around seg_dq's 64-row blocks and the
sort's key width, NRMS_PRECISION_BF16, accumulation, empty inputs, and two invariances.  The cases are named in
tests/segpool_ref.py; tests/test_segpool_ref_host.py shows on the CPU that they sit where they claim to, that the float32 oracle
stays below a quarter of every fp32 bound used here and the split-bf16 statement of the operation below half of every bf16x3 bound.  PARITY UNPINNED, as tests/test_hip_segpool.py: the reference has no such
operation."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import segpool_ref as sr
from tests.test_hip_parity import BF16_GRAD_RTOL, BF16_SCORE_TOL
from tests.test_hip_segpool import OUT_TOL, grad_bound

pytestmark = pytest.mark.gpu

# NRMS_PRECISION_BF16.  The bound the operation needs is 4 x the largest deviation, over sr.BF16_CASES, of pool_ref with the
# projections' operands rounded to bfloat16 from pool_ref, relative to the tensor's scale (out: of max(1, max |out|)): measured on
# the CPU, out 2.1e-3, dx 3.4e-3, dW 2.1e-2, db 4.3e-2, dq 1.45e-2 (docs/EXPERIMENTS.md).  The project's bf16 bars
# (tests/test_hip_parity.py) cover every one of them -- tests/test_segpool_ref_host.py holds them to that -- so these are used.
BF16_TOL = {"out": BF16_SCORE_TOL, "dx": BF16_GRAD_RTOL, "dw": BF16_GRAD_RTOL, "db": BF16_GRAD_RTOL, "dq": BF16_GRAD_RTOL}

FIELDS = ("dx", "dw", "db", "dq")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _autograd_run(c, precision, rows_unique=None):
    from pytorch_news_recommender_amd.segpool import segment_pool
    hx, hw, hb, hq = (_dev(a).requires_grad_(True) for a in (c.x, c.w, c.b, c.qv))
    out = segment_pool(hx, hw, hb, hq, _dev(c.ptr), _dev(c.idx), precision=precision, rows_unique=c.partition if rows_unique is None else rows_unique)
    (out * _dev(c.dout)).sum().backward()
    return sr.Ref(out.detach().cpu(), None, hx.grad.cpu(), hw.grad.cpu(), hb.grad.cpu(), hq.grad.cpu())


def _check(name, precision, got, ref=None, what=""):
    """out within OUT_TOL of max(1, max |out|), every gradient within grad_bound, elementwise (tests/test_hip_segpool.py); for
    NRMS_PRECISION_BF16 within BF16_TOL of the tensor's scale.  Prints the largest error as a fraction of its bound."""
    ref = sr.reference(name) if ref is None else ref
    line = "segpool %-16s %-6s %s" % (name, precision, what)
    bad = []
    scale = max(1.0, float(np.abs(ref.out).max()))
    err = float((got.out.double() - torch.from_numpy(ref.out)).abs().max()) if ref.out.size else 0.0
    tol = (BF16_TOL["out"] if precision == "bf16" else OUT_TOL[precision]) * scale
    line += " out %.2e/%.2e" % (err, tol)
    if not err < tol:
        bad.append("out")
    for f in FIELDS:
        r = torch.from_numpy(getattr(ref, f))
        diff = (getattr(got, f).double() - r).abs()
        bound = BF16_TOL[f] * r.abs().max() + 1e-9 if precision == "bf16" else grad_bound(r)
        ratio = float((diff / bound).max()) if diff.numel() else 0.0
        line += "  %s %.2e (%.3f of bound)" % (f, float(diff.max()) if diff.numel() else 0.0, ratio)
        if not ratio <= 1.0:
            bad.append(f)
    print(line)
    assert not bad, (name, precision, bad, line)


def _unnamed_rows(c):
    return torch.from_numpy(np.bincount(c.idx, minlength=c.R) == 0)


# ---- segment lengths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", ["len_part_20", "len_part_300", "len_shared_20", "len_shared_300"])
def test_segments_of_every_length_around_the_wavefront_and_the_four_member_step(name, precision):
    """One call with segments of 0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 257 and 1000 members."""
    c = sr.case(name)
    got = _autograd_run(c, precision)
    _check(name, precision, got)
    assert bool((got.out[np.diff(c.ptr) == 0] == 0).all())
    if c.partition:
        assert bool((got.dx[_unnamed_rows(c)] == 0).all())


def test_a_thousand_members_that_are_one_row():
    from pytorch_news_recommender_amd.segpool import SegmentPool
    c = sr.case("same_row")
    op = SegmentPool(c.d, c.q, "fp32", rows_unique=False)
    out = op.forward(_dev(c.x), _dev(c.w), _dev(c.b), _dev(c.qv), _dev(c.ptr), _dev(c.idx))
    alpha = op._saved[4][:1000].cpu()
    assert bool((alpha == alpha[0]).all()) and abs(float(alpha[0]) - 1e-3) < 1e-9          # exp(0) = 1, sum = 1000: both exact
    row = torch.from_numpy(c.x[1])
    err = float((out[0].cpu() - row).abs().max())
    print("segpool same_row: out err %.2e" % err)
    assert err < OUT_TOL["fp32"] * max(1.0, float(row.abs().max()))
    _check("same_row", "fp32", _autograd_run(c, "fp32"))


# ---- fan-in: the sorted-span path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", ["fan_a_20", "fan_a_300", "fan_b_20", "fan_b_300"])
def test_rows_whose_runs_sit_in_every_situation_of_the_span_path(name, precision):
    """tests/test_segpool_ref_host.py::test_fanin_layouts_sit_where_the_span_path_branches states which run is where."""
    c = sr.case(name)
    got = _autograd_run(c, precision)
    _check(name, precision, got)
    nobody = _unnamed_rows(c)
    assert int(nobody.sum()) == 1 and bool((got.dx[nobody] == 0).all())


# ---- capacity: desc.nnz beyond seg_ptr[n_seg] -------------------------------------------------------------------------------------
def _abi_run(c, precision, extra, poison, ptr_idx=None):
    """Through the C ABI with desc.nnz = real length + extra; the tail of idx holds PAD_IDX, alpha and the workspace are poisoned
    (the workspace again before the backward: it is no saved state)."""
    from pytorch_news_recommender_amd import _lib
    from tests.guarded import Guarded
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_seg, nnz = len(c.ptr) - 1, len(c.idx)
    cap = nnz + extra
    desc = _lib.SegPoolDesc(n_rows=c.R, n_seg=n_seg, nnz=cap, d=c.d, q=c.q, precision=_lib.PRECISIONS[precision],
                            flags=_lib.NRMS_SEGPOOL_ROWS_UNIQUE if c.partition else 0)
    need = int(lib.nrms_segment_pool_workspace_bytes(C.byref(desc)))
    assert need > 0
    x, w, b, qv, dout = (_dev(a) for a in (c.x, c.w, c.b, c.qv, c.dout))
    if ptr_idx is None:
        ptr, idx = _dev(c.ptr), _dev(np.concatenate([c.idx, np.full(extra, sr.PAD_IDX, np.int32)]))
    else:
        ptr, idx = ptr_idx
    assert idx.numel() == cap
    ws, alpha = Guarded(need, torch.uint8, poison), Guarded(cap * 4, torch.float32, poison)
    t, logit = torch.empty(c.R, c.q, device="cuda"), torch.empty(c.R, device="cuda")
    out, dx = torch.empty(n_seg, c.d, device="cuda"), torch.empty(c.R, c.d, device="cuda")
    dw, db, dq = torch.zeros(c.q, c.d, device="cuda"), torch.zeros(c.q, device="cuda"), torch.zeros(c.q, device="cuda")
    p = _lib.ptr
    _lib.check(lib.nrms_segment_pool_fwd(C.byref(desc), p(x), p(w), p(b), p(qv), p(ptr), p(idx), p(t), p(logit), alpha.ptr, p(out), ws.ptr,
                                         C.c_size_t(need), stream), "nrms_segment_pool_fwd")
    ws.fill(poison)
    _lib.check(lib.nrms_segment_pool_bwd(C.byref(desc), p(x), p(w), p(qv), p(ptr), p(idx), p(t), alpha.ptr, p(dout), p(dx), p(dw), p(db), p(dq),
                                         ws.ptr, C.c_size_t(need), stream), "nrms_segment_pool_bwd")
    torch.cuda.synchronize()
    ws.assert_intact("workspace"), alpha.assert_intact("alpha")
    return sr.Ref(out.cpu(), alpha.view[:nnz].cpu(), dx.cpu(), dw.cpu(), db.cpu(), dq.cpu())


@pytest.mark.parametrize("name,precision", [("fan_a_20", "fp32"), ("fan_a_300", "bf16x3"), ("fan_b_20", "bf16x3"), ("fan_b_300", "fp32"),
                                            ("len_part_20", "fp32"), ("len_part_300", "bf16x3"), ("len_shared_20", "fp32")])
def test_capacity_beyond_the_real_length_changes_no_bit(name, precision):
    """desc.nnz 100 above seg_ptr[n_seg]: the stable sort puts the padding after every live entry, so every addition happens in
    the same order as with the exact length."""
    c = sr.case(name)
    exact, roomy = _abi_run(c, precision, 0, 0xFF), _abi_run(c, precision, 100, 0x7F)
    for f in ("out", "alpha") + FIELDS:
        assert torch.equal(getattr(exact, f), getattr(roomy, f)), (name, precision, f)
    _check(name, precision, roomy, what="capacity +100")


def test_lists_built_on_the_device_from_padded_neighbour_lists():
    """nrms_csr_from_padded -> nrms_segment_pool with nnz = n_seg * K, against the host-built lists of exactly the real length."""
    from pytorch_news_recommender_amd import _lib
    lib = _lib.load()
    c = sr.case("padded_lists")
    lists = sr.padded_lists()
    n_seg, K = lists.shape
    ptr = torch.full((n_seg + 1,), -1, dtype=torch.int32, device="cuda")
    idx = torch.full((n_seg * K,), sr.PAD_IDX, dtype=torch.int32, device="cuda")
    _lib.check(lib.nrms_csr_from_padded(C.c_int64(n_seg), K, _lib.ptr(_dev(lists)), C.c_int64(c.R), _lib.ptr(ptr), _lib.ptr(idx),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nrms_csr_from_padded")
    assert np.array_equal(ptr.cpu().numpy(), c.ptr) and np.array_equal(idx.cpu().numpy()[:len(c.idx)], c.idx)
    assert bool((idx[len(c.idx):] == sr.PAD_IDX).all())
    for precision in ("fp32", "bf16x3"):
        exact = _abi_run(c, precision, 0, 0xFF)
        roomy = _abi_run(c, precision, n_seg * K - len(c.idx), 0x7F, ptr_idx=(ptr, idx))
        for f in ("out", "alpha") + FIELDS:
            assert torch.equal(getattr(exact, f), getattr(roomy, f)), (precision, f)
        _check("padded_lists", precision, roomy, what="capacity n_seg * K")


# ---- widths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("d,q", sr.WIDTHS)
def test_widths_where_a_lane_gains_or_loses_a_column(d, q, precision):
    """d / 4 = 1, 63, 64, 65, 255, 256 (lane l owns float4 columns l + 64 j, j < 4); q = 4, 252, 256, 260, 512 (seg_logit strides
    by 256); the two corners."""
    name = "width_%d_%d" % (d, q)
    _check(name, precision, _autograd_run(sr.case(name), precision))


# ---- row counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("nnz", sr.ROW_NNZ)
@pytest.mark.parametrize("n_rows", sr.ROW_COUNTS)
def test_row_counts_around_the_64_row_blocks_and_the_sort_key_width(n_rows, nnz, precision):
    """seg_dq works in 64-row blocks; the padding key of the sort is n_rows itself, one bit more when n_rows is a power of two."""
    name = "rows_%d_%d" % (n_rows, nnz)
    _check(name, precision, _autograd_run(sr.case(name), precision))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_partition_with_rows_that_belong_to_nobody(precision):
    c = sr.case("rows_orphans")
    got = _autograd_run(c, precision)
    _check("rows_orphans", precision, got)
    assert int(_unnamed_rows(c).sum()) == 9 and bool((got.dx[_unnamed_rows(c)] == 0).all())


# ---- NRMS_PRECISION_BF16 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sr.BF16_CASES)
def test_plain_bf16_projections(name):
    _check(name, "bf16", _autograd_run(sr.case(name), "bf16"))


# ---- accumulation and empties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fan_a_20", "rows_orphans"])
def test_parameter_gradients_are_accumulated(name):
    """dw_add, db_add, dq_vec hold prefill + gradient.  The prefill has the gradient's own scale, so that the rounding of the sum
    (2^-24 of the larger term) stays three orders below grad_bound's 2e-5 of that scale."""
    from pytorch_news_recommender_amd.segpool import SegmentPool
    c, ref = sr.case(name), sr.reference(name)
    op = SegmentPool(c.d, c.q, "fp32", rows_unique=c.partition)
    w, qv = _dev(c.w), _dev(c.qv)
    op.forward(_dev(c.x), w, _dev(c.b), qv, _dev(c.ptr), _dev(c.idx))
    gen = torch.Generator().manual_seed(5)
    pre = {f: torch.randn(getattr(ref, f).shape, generator=gen) * float(np.abs(getattr(ref, f)).max()) for f in ("dw", "db", "dq")}
    acc = {f: v.clone().cuda() for f, v in pre.items()}
    dx = op.backward(w, qv, _dev(c.dout), acc["dw"], acc["db"], acc["dq"])
    for f in ("dw", "db", "dq"):
        r = torch.from_numpy(getattr(ref, f))
        diff = (acc[f].cpu().double() - (pre[f].double() + r)).abs()
        assert bool((diff <= grad_bound(r)).all()), (name, f, float(diff.max()))
    assert bool(((dx.cpu().double() - torch.from_numpy(ref.dx)).abs() <= grad_bound(torch.from_numpy(ref.dx))).all())


@pytest.mark.parametrize("rows_unique", [True, False], ids=["partition", "shared_rows"])
def test_no_segment_at_all(rows_unique):
    from pytorch_news_recommender_amd.segpool import SegmentPool
    c = sr.case("rows_orphans")
    op = SegmentPool(c.d, c.q, "fp32", rows_unique=rows_unique)
    w, qv = _dev(c.w), _dev(c.qv)
    out = op.forward(_dev(c.x), w, _dev(c.b), qv, torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert out.shape == (0, c.d)
    gen = torch.Generator().manual_seed(6)
    pre = [torch.randn(s, generator=gen) for s in ((c.q, c.d), (c.q,), (c.q,))]
    acc = [v.clone().cuda() for v in pre]
    dx = op.backward(w, qv, torch.zeros(0, c.d, device="cuda"), *acc)
    torch.cuda.synchronize()
    for a, v in zip(acc, pre):
        assert torch.equal(a.cpu(), v)
    assert dx.shape == (c.R, c.d) and bool((dx == 0).all())


@pytest.mark.parametrize("rows_unique", [True, False], ids=["partition", "shared_rows"])
def test_every_segment_empty(rows_unique):
    from pytorch_news_recommender_amd.segpool import SegmentPool
    c = sr.case("rows_orphans")
    op = SegmentPool(c.d, c.q, "bf16x3", rows_unique=rows_unique)
    w, qv = _dev(c.w), _dev(c.qv)
    out = op.forward(_dev(c.x), w, _dev(c.b), qv, torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert out.shape == (7, c.d) and bool((out == 0).all())
    acc = [torch.zeros(c.q, c.d, device="cuda"), torch.zeros(c.q, device="cuda"), torch.zeros(c.q, device="cuda")]
    dx = op.backward(w, qv, torch.ones(7, c.d, device="cuda"), *acc)
    assert bool((dx == 0).all()) and all(bool((a == 0).all()) for a in acc)


# ---- invariances ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["len_shared_20", "rows_orphans"])
def test_the_order_of_the_segments_does_not_change_a_bit_of_out(name):
    from pytorch_news_recommender_amd.segpool import SegmentPool
    c = sr.case(name)
    n_seg = len(c.ptr) - 1
    perm = np.random.default_rng(8).permutation(n_seg)
    ptr2 = np.concatenate([[0], np.cumsum(np.diff(c.ptr)[perm])]).astype(np.int32)
    idx2 = np.concatenate([c.idx[c.ptr[s]:c.ptr[s + 1]] for s in perm]).astype(np.int32)
    outs = []
    for ptr, idx in ((c.ptr, c.idx), (ptr2, idx2)):
        op = SegmentPool(c.d, c.q, "bf16x3", rows_unique=c.partition)
        outs.append(op.forward(_dev(c.x), _dev(c.w), _dev(c.b), _dev(c.qv), _dev(ptr), _dev(idx)).cpu())
    assert torch.equal(outs[0][perm], outs[1])


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_a_partition_with_and_without_the_rows_unique_flag(precision):
    """The forward does not look at the flag: the same bits.  The two backward paths add in different orders: each within
    grad_bound of the reference."""
    from pytorch_news_recommender_amd.segpool import SegmentPool
    c = sr.case("len_part_20")
    res, grads = [], []
    for unique in (True, False):
        op = SegmentPool(c.d, c.q, precision, rows_unique=unique)
        out = op.forward(_dev(c.x), _dev(c.w), _dev(c.b), _dev(c.qv), _dev(c.ptr), _dev(c.idx)).cpu()
        res.append((out, op._saved[4][:len(c.idx)].cpu()))
        grads.append(_autograd_run(c, precision, rows_unique=unique))
        _check("len_part_20", precision, grads[-1], what="rows_unique=%s" % unique)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(grads[0].out, grads[1].out)
    for f in FIELDS:
        diff = (getattr(grads[0], f).double() - getattr(grads[1], f).double()).abs()
        assert bool((diff <= grad_bound(torch.from_numpy(getattr(sr.reference("len_part_20"), f)))).all()), f
