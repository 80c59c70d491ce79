"""Float64 statement of nrms_segment_pool_fwd / _bwd (include/nrms_hip.h; csrc/segpool.hip), builders for index lists that sit
where its kernels change behaviour, and the named cases of tests/test_hip_segpool_edges.py.  Import-safe on the CPU, no GPU
use: tests/test_segpool_ref_host.py holds pool_ref against autograd through oracle/segpool_oracle.py and checks that the cases
sit where they claim to.

The backward of a list whose rows are shared (no NRMS_SEGPOOL_ROWS_UNIQUE) sorts the list entries by row, stably, and walks the
sorted entries in spans of SEG_SPAN = 64 positions.  Row r's run is therefore the sorted positions
[sum(mult[:r]), sum(mult[:r + 1])), mult[r] = how often the lists name r: the multiplicities place every run exactly
(fanin_layout), and span_classes restates the kernel's arithmetic on them."""
import collections
import functools

import numpy as np

SEG_SPAN = 64                                     # csrc/segpool.hip
PAD_IDX = 0x7f7f7f7f                              # what the tests put into idx beyond the lists' real length

SPAN_CLASSES = ("owned", "slot0", "slot1", "inner", "ends_on_boundary", "padded_tail")

Ref = collections.namedtuple("Ref", "out alpha dx dw db dq")
Case = collections.namedtuple("Case", "name R d q partition x w b qv ptr idx dout")


def bf16_round(a):
    """float64 -> the nearest bfloat16 (ties to even), as float64."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(a))


def _split(a):
    hi = bf16_round(a)
    return hi, bf16_round(a - hi)


def _product(operands):
    """A B as the projections of the given precision form it, with exact accumulation.  bf16: both operands rounded to bfloat16.
    bf16x3: each operand hi + lo, hi = bf16(x), lo = bf16(x - hi) (16 significant bits), A B = hi hi + hi lo + lo hi
    (csrc/gemm_bf16.hip)."""
    if operands == "exact":
        return lambda A, B: A @ B
    if operands == "bf16":
        return lambda A, B: bf16_round(A) @ bf16_round(B)
    assert operands == "bf16x3", operands

    def mm(A, B):
        (ah, al), (bh, bl) = _split(A), _split(B)
        return ah @ bh + ah @ bl + al @ bh
    return mm


def pool_ref(x, w, b, q, seg_ptr, idx, dout, operands="exact"):
    """out [n_seg, d], alpha [nnz] and the gradients of sum(out * dout) with respect to x, W_add, b_add, q_vec, in float64
    (closed form, no loop over segments or members).  operands "bf16" / "bf16x3": the operands of the three projections -- x and
    W in x W^T, dZ, W and x in dZ W and dZ^T [x | 1] -- carry that precision (_product) and nothing else does: what
    NRMS_PRECISION_BF16 / _BF16X3 do, with exact accumulation."""
    x, w, b, q, dout = (np.asarray(a, dtype=np.float64) for a in (x, w, b, q, dout))
    ptr, idx = np.asarray(seg_ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    R, d = x.shape
    n_seg = len(ptr) - 1
    idx = idx[:int(ptr[-1])]
    mm = _product(operands)
    T = np.tanh(mm(x, w.T) + b)
    logit = T @ q
    seg_of = np.repeat(np.arange(n_seg), np.diff(ptr))
    lg = logit[idx]
    mx = np.full(n_seg, -np.inf)
    np.maximum.at(mx, seg_of, lg)
    e = np.exp(lg - mx[seg_of])
    alpha = e / np.bincount(seg_of, e, n_seg)[seg_of]
    A = np.zeros((n_seg, R))                                        # A[s][r] = sum of alpha over the entries of s that name r
    np.add.at(A, (seg_of, idx), alpha)
    out = A @ x
    dalpha = np.einsum("kd,kd->k", dout[seg_of], x[idx])
    dlogit = alpha * (dalpha - np.bincount(seg_of, alpha * dalpha, n_seg)[seg_of])
    da = np.bincount(idx, dlogit, R)
    dq = T.T @ da
    dZ = da[:, None] * q[None, :] * (1.0 - T * T)
    dwb = mm(dZ.T, np.concatenate([x, np.ones((R, 1))], 1))
    dx = mm(dZ, w) + A.T @ dout
    return Ref(out, alpha, dx, dwb[:, :d], dwb[:, d], dq)


def lengths_layout(lengths, partition, seed, n_rows=None):
    """seg_ptr, idx (int32) with exactly these segment lengths.  partition: every row is named once at most (n_rows >=
    sum(lengths); the rows beyond it belong to nobody), in a shuffled order.  Otherwise every entry is drawn from all n_rows rows:
    repeats across and inside segments."""
    rng = np.random.default_rng(seed)
    lengths = [int(n) for n in lengths]
    nnz = sum(lengths)
    if partition:
        n_rows = nnz if n_rows is None else n_rows
        assert n_rows >= nnz
        idx = rng.permutation(n_rows)[:nnz]
    else:
        assert n_rows is not None and (n_rows > 0 or nnz == 0)
        idx = rng.integers(0, max(n_rows, 1), nnz)
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), idx.astype(np.int32)


def fanin_layout(mult, seed):
    """seg_ptr, idx (int32): the multiset {r repeated mult[r] times}, shuffled, cut into segments of random length 1 .. 90
    (in-segment repeats happen).  len(mult) rows."""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(np.repeat(np.arange(len(mult)), mult))
    ptr = [0]
    while ptr[-1] < len(idx):
        ptr.append(min(len(idx), ptr[-1] + int(rng.integers(1, 91))))
    return np.asarray(ptr, np.int32), idx.astype(np.int32)


def span_classes(mult):
    """One set per row: where its run of sorted entries lies among the spans, by the arithmetic of seg_span_gather_kernel and
    seg_row_combine_kernel.
      owned             the run lies in one span, which adds it to dx itself
      slot0             it starts at a span's first position and leaves that span (partial slot 0 of the span)
      slot1             it starts later in a span and leaves it (slot 1)
      inner             a span lies wholly inside it, between the one it starts and the one it ends in
      ends_on_boundary  its last entry is a span's last position (the run ends without a next entry in the span)
      padded_tail       padding follows it in its last span (the last run of lists whose length is no multiple of 64)
    A row nobody names has no run: an empty set."""
    res, p0 = [], 0
    total = sum(int(m) for m in mult)
    for m in mult:
        m = int(m)
        p1 = p0 + m
        c = set()
        if m > 0:
            sa, sb = p0 // SEG_SPAN, (p1 - 1) // SEG_SPAN
            if sa == sb:
                c.add("owned")
            else:
                c.add("slot0" if p0 % SEG_SPAN == 0 else "slot1")
                if sb - sa >= 2:
                    c.add("inner")
            if p1 % SEG_SPAN == 0:
                c.add("ends_on_boundary")
            if p1 == total and total % SEG_SPAN != 0:
                c.add("padded_tail")
        res.append(frozenset(c))
        p0 = p1
    return res


# ---- the cases of tests/test_hip_segpool_edges.py -------------------------------------------------------------------------------
LENGTHS = (129, 1, 1000, 0, 3, 64, 255, 4, 63, 5, 127, 65, 257, 128)          # 2 101 members
FANIN = {
    # runs [0,64) [64,65) [65,128) [128,193) [193,256) [256,384) none [384,584) [584,585) [585,712) [712,776) [776,779): 779 of 832
    "fan_a": (64, 1, 63, 65, 63, 128, 0, 200, 1, 127, 64, 3),
    # runs [0,10) [10,64) [64,128) [128,258) [258,320) none [320,512) [512,576) [576,577) [577,704) [704,768): no padding
    "fan_b": (10, 54, 64, 130, 62, 0, 192, 64, 1, 127, 64),
}
WIDTHS = [(d, 8) for d in (4, 252, 256, 260, 1020, 1024)] + [(20, q) for q in (4, 252, 256, 260, 512)] + [(1024, 512), (4, 4)]
ROW_COUNTS = (1, 63, 64, 65, 127, 128, 129)
ROW_NNZ = (128, 100)                              # a multiple of 64 and not
DOUT_SCALE = 1e-2                                 # (tests/test_hip_segpool.py)
# Where every member of every segment is the same row, d(logit) -- and with it dW, db, dq -- is zero in exact arithmetic and rounding
# noise in any other: a serial float32 sum of n equal terms is off by up to n 2^-24 of itself, and that error, times |dout|, is what
# reaches these gradients, while grad_bound is its absolute floor, 1e-9.  With n = 1000 and this dout the worst case is 6e-10.
DOUT_SCALE_ONE_ROW = 1e-5


# W_SCALE_NOTE.  d(b_add)[n] = -q[n] sum_r d(logit_r) T[r][n]^2, because the d(logit) of a segment sum to zero.  With the Xavier range
# of tests/test_hip_segpool.py::_case the projection at d = 20, q = 512 has a deviation of 0.14, T^2 is about 0.02, and db is a
# fiftieth of its own terms: split-bf16 operands (16 significant bits) with EXACT accumulation are then at 1.39 of grad_bound's
# 2e-5 of max |db|, and the kernel, which does just that, at 1.19.  W is drawn so that the projection's deviation is 0.5 at
# every (d, q) -- what the Xavier range gives at (300, 200) -- and tests/test_segpool_ref_host.py holds the split-bf16 statement of
# every case below a quarter of the bounds, as it holds the float32 oracle.
def _inputs(R, n_seg, d, q, seed, dout_scale=DOUT_SCALE):
    """The distributions of tests/test_hip_segpool.py::_case, but for W (W_SCALE_NOTE)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((R, d)) * 0.5).astype(np.float32)
    w = (rng.uniform(-1, 1, (q, d)) * np.sqrt(3.0 / d)).astype(np.float32)               # x W^T ~ 0.5 at every width, see W_SCALE_NOTE
    b = rng.uniform(-0.05, 0.05, q).astype(np.float32)
    qv = rng.uniform(-0.1, 0.1, q).astype(np.float32)
    dout = (rng.standard_normal((n_seg, d)) * dout_scale).astype(np.float32)
    return x, w, b, qv, dout


def _make(name, R, d, q, partition, ptr, idx, seed):
    one_row = len(set(np.asarray(idx).tolist())) == 1
    x, w, b, qv, dout = _inputs(R, len(ptr) - 1, d, q, seed, DOUT_SCALE_ONE_ROW if one_row else DOUT_SCALE)
    return Case(name, R, d, q, partition, x, w, b, qv, ptr, idx, dout)


def _lengths_summing_to(nnz, seed):
    """Segment lengths 0 .. 39 (the range of the existing tests), the last one cut so that they sum to nnz."""
    rng, out = np.random.default_rng(seed), []
    while sum(out) < nnz:
        out.append(min(nnz - sum(out), 0 if len(out) % 7 == 3 else int(rng.integers(1, 40))))
    return out


def case_names():
    names = ["len_%s_%d" % (m, d) for m in ("part", "shared") for d in (20, 300)] + ["same_row"]
    names += ["%s_%d" % (f, d) for f in FANIN for d in (20, 300)] + ["padded_lists"]
    names += ["width_%d_%d" % dq for dq in WIDTHS]
    names += ["rows_%d_%d" % (r, n) for r in ROW_COUNTS for n in ROW_NNZ] + ["rows_orphans"]
    return names


# another draw for the cases whose first one left the split-bf16 statement above 0.4 of a bound (tests/test_segpool_ref_host.py asserts 0.5)
SEED_SALT = {"rows_orphans": 1, "width_20_512": 1}


@functools.lru_cache(maxsize=None)
def case(name):
    """A named case (arrays: treat them as read-only, they are shared)."""
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(name)) + SEED_SALT.get(name, 0)
    k = name.split("_")
    if k[0] == "len":
        d = int(k[2])
        part = k[1] == "part"
        R = sum(LENGTHS) + 9 if part else 300                      # partition: nine rows that belong to nobody
        ptr, idx = lengths_layout(LENGTHS, part, seed, R)
        return _make(name, R, d, {20: 8, 300: 200}[d], part, ptr, idx, seed)
    if name == "same_row":
        ptr, idx = np.asarray([0, 1000], np.int32), np.full(1000, 1, np.int32)
        return _make(name, 3, 20, 8, False, ptr, idx, seed)
    if k[0] == "fan":
        mult, d = FANIN[k[0] + "_" + k[1]], int(k[2])
        ptr, idx = fanin_layout(mult, seed)
        return _make(name, len(mult), d, {20: 8, 300: 200}[d], False, ptr, idx, seed)
    if name == "padded_lists":
        lists = padded_lists()
        keep = lists >= 0
        ptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int32)
        return _make(name, 64, 20, 8, False, ptr, lists[keep].astype(np.int32), seed)
    if k[0] == "width":
        ptr, idx = lengths_layout(_lengths_summing_to(700, seed), False, seed, 64)
        return _make(name, 64, int(k[1]), int(k[2]), False, ptr, idx, seed)
    if name == "rows_orphans":
        ptr, idx = lengths_layout(_lengths_summing_to(120, seed), True, seed, 129)
        return _make(name, 129, 20, 8, True, ptr, idx, seed)
    if k[0] == "rows":
        R, nnz = int(k[1]), int(k[2])
        ptr, idx = lengths_layout(_lengths_summing_to(nnz, seed), False, seed, R)
        return _make(name, R, 20, 8, False, ptr, idx, seed)
    raise KeyError(name)


def padded_lists(n_seg=40, K=24, n_rows=64, seed=77):
    """[n_seg, K] int64 neighbour lists with -1 holes (the input of nrms_csr_from_padded); one list is all holes."""
    rng = np.random.default_rng(seed)
    lists = rng.integers(0, n_rows, (n_seg, K)).astype(np.int64)
    lists[rng.random((n_seg, K)) < 0.35] = -1
    lists[5] = -1
    return lists


@functools.lru_cache(maxsize=None)
def reference(name, operands="exact"):
    c = case(name)
    return pool_ref(c.x, c.w, c.b, c.qv, c.ptr, c.idx, c.dout, operands)


# ---- NRMS_PRECISION_BF16 ---------------------------------------------------------------------------------------------------------
BF16_CASES = ("len_part_300", "len_shared_300", "fan_a_20", "fan_a_300")


def bf16_deviation(name):
    """{tensor: max |pool_ref with bf16 operands - pool_ref| / max |pool_ref|} (out: over max(1, max |out|), the scale of OUT_TOL)."""
    a, r = reference(name), reference(name, "bf16")
    dev = {}
    for f in ("out", "dx", "dw", "db", "dq"):
        ea, er = getattr(a, f), getattr(r, f)
        scale = float(np.abs(ea).max())
        dev[f] = float(np.abs(er - ea).max()) / (max(1.0, scale) if f == "out" else scale)
    return dev
