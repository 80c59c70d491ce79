"""nrms_pooled_ce_fwd_bwd (csrc/poolce.hip) through the C ABI against the float64 restatement of tests/pooled_ce_ref.py.

Shapes.  B in {1, 2, 31, 32, 33, 65} x C in {1, 2, 5}, each pair twice with d cycling through {1, 2, 3, 63, 64, 65, 300} and R through
{0, 1, 50}; one case at B = 512, C = 5, d = 300, R = 50; and the edges of the kernels' tiles: 32 rows x 128 columns per workgroup
(M = B*C at 127 / 128 / 129, d as the column extent of the gradient products at 127 / 128 / 129), K stages of 32 (d = 31 / 32 / 33),
64 reject entries per LDS chunk (R = 63 / 64 / 65 / 256), one K slab of duser per 512 pool columns (M = 512 / 513 / 515, and
M = 4608: 8 slabs of 576, not 9 of 512), d = 1024.  Every case runs the masks NULL, random, one row whose positive is masked, and one column
group dead for everyone, with col_bias NULL or given in turn.

Inputs.  Vectors are N(0, 1) d^-1/4, so scores are O(1) as a trained model's are; ids come from a range of about M / 2 values, so
pool columns repeat rows' positives and appear in reject lists; reject lists hold padding zeros, and some pool slots hold id 0.

Bound (the rule of tests/test_hip_step_tail.py for cross-entropy; no invented tolerance).  A torch fp32 restatement (mm,
compare-mask, log_softmax, two mm) runs on the CPU on the same inputs; T is its largest error against float64 over an output
tensor.  Per element the kernel is allowed 4 T + A + one fp32 ulp of the reference value, A = (K + 8) 2^-24 sum |terms| of the
element's final sum in float64 (K = M for duser, B for dcand, B for the row losses in loss_sum): the kernel's own summation order.
Every test prints its largest error beside its bound (docs/EXPERIMENTS.md records them)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from tests.guarded import POISONS, Pool, assert_same_bits
from tests.pooled_ce_ref import pooled_ce

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
EINVAL = _lib.NRMS_EINVAL
DS, RS = (1, 2, 3, 63, 64, 65, 300), (0, 1, 50)
MASKS = ("null", "random", "row_dead", "group_dead")


def _grid_cases():
    out = []
    for i, (B, Cn) in enumerate(itertools.product((1, 2, 31, 32, 33, 65), (1, 2, 5))):
        out.append((B, Cn, DS[i % 7], RS[i % 3]))
        out.append((B, Cn, DS[(i + 3) % 7], RS[(i + 1) % 3]))
    return out


EDGE_CASES = [(127, 1, 5, 0), (128, 1, 33, 1), (129, 1, 31, 63), (43, 3, 32, 64), (64, 2, 127, 65), (5, 5, 128, 256), (7, 3, 129, 2),
              (256, 2, 8, 3), (171, 3, 6, 0), (103, 5, 20, 5), (72, 64, 4, 1), (3, 2, 1024, 7)]
CASES = _grid_cases() + EDGE_CASES


def lib():
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def make_mask(kind, B, Cn, rng):
    if kind == "null":
        return None
    m = np.ones((B, Cn), dtype=np.uint8)
    if kind == "random":
        m = (rng.random((B, Cn)) < 0.7).astype(np.uint8)
    elif kind == "row_dead":
        m[B // 2, 0] = 0
    elif Cn > 1:
        m[:, Cn - 1] = 0
    else:
        m[::2] = 0
    return m


def make_inputs(B, Cn, d, R, seed, mask_kind="null", bias=False):
    rng = np.random.default_rng(seed)
    M = B * Cn
    s = float(d) ** -0.25
    x = dict(B=B, C=Cn, d=d, R=R)
    x["cand"] = (rng.standard_normal((M, d)) * s).astype(np.float32)
    x["user"] = (rng.standard_normal((B, d)) * s).astype(np.float32)
    n_ids = max(4, M // 2)
    ids = rng.integers(1, n_ids + 1, size=M).astype(np.int64)
    ids[rng.random(M) < 0.05] = 0                                             # padding ids in the pool: a reject entry 0 must not match
    x["ids"] = ids
    x["mask"] = make_mask(mask_kind, B, Cn, rng)
    rej = None
    if R:
        rej = rng.integers(1, n_ids + 1, size=(B, R)).astype(np.int64)
        rej[rng.random((B, R)) < 0.3] = 0
        rej[rng.random((B, R)) < 0.02] = -3
    x["reject"] = rej
    x["bias"] = (rng.standard_normal(M) * 2.0).astype(np.float32) if bias else None
    return x


def reference(x, gs):
    return pooled_ce(x["cand"], x["user"], x["ids"], x["C"], None if x["mask"] is None else x["mask"].reshape(-1), x["reject"], x["bias"],
                     float(np.float32(gs)))


def torch_restatement(x, inc, gs, dtype=torch.float32):
    """mm, compare-mask (taken from the restatement: it is integer logic), log_softmax, two mm; on the CPU."""
    B, Cn = x["B"], x["C"]
    c, u = torch.from_numpy(x["cand"]).to(dtype), torch.from_numpy(x["user"]).to(dtype)
    z = u @ c.T
    if x["bias"] is not None:
        z = z + torch.from_numpy(x["bias"]).to(dtype)[None, :]
    inc_t = torch.from_numpy(inc)
    own = torch.arange(B) * Cn
    live = inc_t[torch.arange(B), own]
    zm = torch.where(inc_t, z, torch.full_like(z, float("-inf")))
    g = torch.zeros_like(z)
    loss = torch.zeros(B, dtype=dtype)
    if bool(live.any()):
        lsm = torch.log_softmax(zm[live], dim=1)
        rows = torch.arange(int(live.sum()))
        loss[live] = -lsm[rows, own[live]]
        p = torch.exp(lsm)
        p[rows, own[live]] -= 1.0
        g[live] = torch.where(inc_t[live], p * torch.tensor(float(np.float32(gs)), dtype=dtype), torch.zeros_like(p))
    return dict(loss_sum=float(loss.sum()), duser=(g @ c).numpy().astype(np.float64), dcand=(g.T @ u).numpy().astype(np.float64))


def bounds(x, ref, gs):
    t = torch_restatement(x, ref["inc"], gs)
    B, M = x["B"], x["B"] * x["C"]
    T = dict(loss=abs(t["loss_sum"] - ref["loss_sum"]), duser=float(np.abs(t["duser"] - ref["duser"]).max()),
             dcand=float(np.abs(t["dcand"] - ref["dcand"]).max()))
    allow = dict(loss=4 * T["loss"] + (B + 8) * U24 * float(np.abs(ref["loss"]).sum()) + float(ulp32(ref["loss_sum"])),
                 duser=4 * T["duser"] + (M + 8) * U24 * ref["abs_duser"] + ulp32(ref["duser"]),
                 dcand=4 * T["dcand"] + (B + 8) * U24 * ref["abs_dcand"] + ulp32(ref["dcand"]))
    return T, allow


def call(x, gs, poison=0xFF, want_grad=True, ws_delta=0, only=None):
    """One call with every buffer between guard bands, the workspace at the size the query reports (+ ws_delta).  -> (rc, outputs)."""
    B, Cn, d, R = x["B"], x["C"], x["d"], x["R"]
    M = B * Cn
    need = int(lib().nrms_pooled_ce_workspace_bytes(B, Cn, d, R))
    assert need > 0
    pool = Pool(poison)
    pool.elems("cand", M * d, init=x["cand"])
    pool.elems("user", B * d, init=x["user"])
    pool.elems("ids", M, torch.int64, init=x["ids"])
    if x["mask"] is not None:
        pool.elems("mask", M, torch.uint8, init=x["mask"].reshape(-1))
    if R:
        pool.elems("reject", B * R, torch.int64, init=x["reject"])
    if x["bias"] is not None:
        pool.elems("bias", M, init=x["bias"])
    pool.elems("loss", 1, init="zero")
    pool.elems("pairs", 1, torch.int64, init="zero")
    pool.elems("dcand", M * d)
    pool.elems("duser", B * d)
    pool.new("ws", need + ws_delta)
    snap = pool.snapshot()
    p = lambda name: pool[name].ptr if name in pool.bufs else None
    dc, du = (p("dcand"), p("duser")) if want_grad else (None, None)
    if only == "dcand":
        du = None
    elif only == "duser":
        dc = None
    rc = lib().nrms_pooled_ce_fwd_bwd(B, Cn, d, R, p("cand"), p("user"), p("ids"), p("mask"), p("reject"), p("bias"), C.c_float(gs),
                                      p("loss"), dc, du, p("pairs"), p("ws"), C.c_size_t(need + ws_delta), _stream())
    pool.intact("nrms_pooled_ce_fwd_bwd")
    if rc != 0:
        pool.assert_unchanged(snap, "a refused nrms_pooled_ce_fwd_bwd")
        return rc, None
    for name in ("cand", "user", "ids", "mask", "reject", "bias") + (() if want_grad else ("dcand", "duser")):
        if name in pool.bufs:
            assert pool[name].unchanged_since(snap[name]), "%s was written" % name
    out = dict(loss=pool["loss"].numpy(), pairs=pool["pairs"].numpy())
    if want_grad:
        out["dcand"], out["duser"] = pool["dcand"].numpy((M, d)), pool["duser"].numpy((B, d))
    return rc, out


def check(x, out, ref, gs, tag):
    T, allow = bounds(x, ref, gs)
    k_loss = float(out["loss"][0])
    e = dict(loss=abs(k_loss - ref["loss_sum"]), duser=np.abs(out["duser"] - ref["duser"]), dcand=np.abs(out["dcand"] - ref["dcand"]))
    print("pooled_ce %s: loss torch %.2e kernel %.2e allowed %.2e (ref %.6g) | duser torch %.2e kernel %.2e allowed >= %.2e | "
          "dcand torch %.2e kernel %.2e allowed >= %.2e | pairs %d"
          % (tag, T["loss"], e["loss"], allow["loss"], ref["loss_sum"], T["duser"], float(e["duser"].max()), float(allow["duser"].min()),
             T["dcand"], float(e["dcand"].max()), float(allow["dcand"].min()), ref["n_pairs"]))
    assert np.isfinite(k_loss) and np.isfinite(out["duser"]).all() and np.isfinite(out["dcand"]).all(), tag
    assert int(out["pairs"][0]) == ref["n_pairs"], (tag, int(out["pairs"][0]), ref["n_pairs"])
    assert e["loss"] <= allow["loss"], (tag, k_loss, ref["loss_sum"], e["loss"], allow["loss"])
    assert (e["duser"] <= allow["duser"]).all(), (tag, float((e["duser"] - allow["duser"]).max()))
    assert (e["dcand"] <= allow["dcand"]).all(), (tag, float((e["dcand"] - allow["dcand"]).max()))
    # what is excluded is excluded exactly: a column in nobody's softmax, a dead row
    no_col, no_row = ~ref["inc"].any(axis=0), ~ref["inc"].any(axis=1)
    assert not bits(out["dcand"][no_col]).any(), tag
    assert not bits(out["duser"][no_row]).any(), tag


@pytest.mark.parametrize("B,Cn,d,R", CASES)
def test_pooled_ce_against_float64(B, Cn, d, R):
    case = CASES.index((B, Cn, d, R))
    gs = 1.0 / B
    for mi, kind in enumerate(MASKS):
        x = make_inputs(B, Cn, d, R, seed=1000 * case + mi, mask_kind=kind, bias=(mi + case) % 2 == 1)
        ref = reference(x, gs)
        runs = {}
        for poison in POISONS:
            rc, out = call(x, gs, poison)
            assert rc == 0, lib().nrms_last_error()
            runs[poison] = out
        assert_same_bits(runs, "pooled_ce B=%d C=%d d=%d R=%d %s" % (B, Cn, d, R, kind))
        out = runs[POISONS[0]]
        check(x, out, ref, gs, "B=%d C=%d d=%d R=%d %s%s" % (B, Cn, d, R, kind, " bias" if x["bias"] is not None else ""))
        # doubling grad_scale doubles every gradient bit for bit and leaves the loss alone
        rc, twice = call(x, 2 * gs)
        assert rc == 0
        assert np.array_equal(bits(twice["dcand"]), bits(np.float32(2) * out["dcand"])), kind
        assert np.array_equal(bits(twice["duser"]), bits(np.float32(2) * out["duser"])), kind
        assert np.array_equal(bits(twice["loss"]), bits(out["loss"])), kind
        # loss only: the same loss and count, neither gradient written (call() checks the poisoned buffers)
        rc, alone = call(x, gs, want_grad=False)
        assert rc == 0
        assert np.array_equal(bits(alone["loss"]), bits(out["loss"])) and alone["pairs"][0] == out["pairs"][0], kind


def test_pooled_ce_at_the_training_shape():
    B, Cn, d, R = 512, 5, 300, 50
    gs = 1.0 / B
    x = make_inputs(B, Cn, d, R, seed=77, mask_kind="random", bias=True)
    ref = reference(x, gs)
    rc, out = call(x, gs, 0xFF)
    assert rc == 0, lib().nrms_last_error()
    rc, again = call(x, gs, 0x7F)
    assert rc == 0
    assert_same_bits({0xFF: out, 0x7F: again}, "pooled_ce at B=512 C=5 d=300 R=50")
    check(x, out, ref, gs, "B=512 C=5 d=300 R=50 random bias")


def test_pooled_ce_accumulates_loss_and_pairs():
    x = make_inputs(33, 5, 64, 1, seed=9)
    rc, one = call(x, 1.0)
    assert rc == 0
    B, Cn, d, R = x["B"], x["C"], x["d"], x["R"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cand, user, ids, rej = t(x["cand"]), t(x["user"]), t(x["ids"]), t(x["reject"])
    loss = torch.full((1,), 3.25, dtype=torch.float32, device="cuda")
    pairs = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    need = int(lib().nrms_pooled_ce_workspace_bytes(B, Cn, d, R))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        rc = lib().nrms_pooled_ce_fwd_bwd(B, Cn, d, R, _lib.ptr(cand), _lib.ptr(user), _lib.ptr(ids), None, _lib.ptr(rej), None,
                                          C.c_float(1.0), _lib.ptr(loss), None, None, _lib.ptr(pairs), _lib.ptr(ws), C.c_size_t(need),
                                          _stream())
        assert rc == 0
    v = np.float32(one["loss"][0])
    assert loss.cpu().numpy()[0] == np.float32(np.float32(np.float32(3.25) + v) + v)
    assert int(pairs.cpu()[0]) == 7 + 2 * int(one["pairs"][0])


def test_pooled_ce_refusals():
    x = make_inputs(5, 3, 8, 2, seed=3)
    rc, _ = call(x, 1.0, ws_delta=-1)
    assert rc == EINVAL and b"workspace" in lib().nrms_last_error()
    for only in ("dcand", "duser"):
        rc, _ = call(x, 1.0, only=only)
        assert rc == EINVAL and b"both" in lib().nrms_last_error()
    rc, _ = call(x, 1.0, ws_delta=4096)                                      # a larger workspace is fine
    assert rc == 0
    # outside the domain: refused before anything is read (every pointer is a 16-byte dummy)
    dummy = torch.zeros(4, dtype=torch.float32, device="cuda")
    p = _lib.ptr(dummy)
    for B, Cn, d, R in ((0, 1, 8, 0), (4097, 1, 8, 0), (1, 65, 8, 0), (1, 0, 8, 0), (4096, 9, 8, 0), (2, 2, 0, 0), (2, 2, 1025, 0),
                        (2, 2, 8, 257), (2, 2, 8, -1)):
        assert lib().nrms_pooled_ce_workspace_bytes(B, Cn, d, R) == 0
        rc = lib().nrms_pooled_ce_fwd_bwd(B, Cn, d, R, p, p, p, None, p if R else None, None, C.c_float(1.0), p, p, p, None, p,
                                          C.c_size_t(1 << 40), _stream())
        assert rc == EINVAL and b"pooled_ce" in lib().nrms_last_error(), (B, Cn, d, R)
    # reject is NULL exactly when R == 0
    rc = lib().nrms_pooled_ce_fwd_bwd(2, 2, 8, 0, p, p, p, None, p, None, C.c_float(1.0), p, p, p, None, p, C.c_size_t(1 << 40), _stream())
    assert rc == EINVAL
    rc = lib().nrms_pooled_ce_fwd_bwd(2, 2, 8, 1, p, p, p, None, None, None, C.c_float(1.0), p, p, p, None, p, C.c_size_t(1 << 40), _stream())
    assert rc == EINVAL
    torch.cuda.synchronize()
    assert not dummy.cpu().numpy().any()


@pytest.mark.parametrize("B,Cn,d", [(9, 5, 300), (33, 5, 63), (2, 2, 1), (52, 5, 64)])
@pytest.mark.parametrize("masked", [False, True])
def test_pooled_ce_reduces_to_the_rowwise_kernels(B, Cn, d, masked):
    """Reject lists that name every other row's ids leave each row its own C candidates: the loss and the gradients of
    nrms_click_score_fwd + nrms_ce_loss_fwd_bwd + nrms_click_score_bwd, within the same bound."""
    R = (B - 1) * Cn
    assert R <= 256
    gs = 1.0 / B
    x = make_inputs(B, Cn, d, 0, seed=B + d)
    rng = np.random.default_rng(d)
    M = B * Cn
    x["ids"] = (rng.permutation(M) + 1).astype(np.int64)
    idm = x["ids"].reshape(B, Cn)
    x["reject"] = np.stack([np.delete(idm, b, axis=0).reshape(-1) for b in range(B)]).astype(np.int64) if R else None
    x["R"] = R
    if masked:                                     # negatives only: the row-wise kernels score a masked slot -1e9, whose exp is 0
        m = (rng.random((B, Cn)) < 0.6).astype(np.uint8)
        m[:, 0] = 1
        x["mask"] = m
    ref = reference(x, gs)
    assert ref["n_pairs"] == (B * (Cn - 1) if x["mask"] is None else int(x["mask"].sum()) - B)
    rc, out = call(x, gs)
    assert rc == 0, lib().nrms_last_error()
    check(x, out, ref, gs, "rowwise B=%d C=%d d=%d masked=%d" % (B, Cn, d, masked))
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cand, user, mask = t(x["cand"]), t(x["user"]), t(x["mask"])
    scores = torch.empty(B, Cn, dtype=torch.float32, device="cuda")
    _lib.check(lib().nrms_click_score_fwd(B, Cn, d, _lib.ptr(cand), _lib.ptr(user), _lib.ptr(mask), _lib.ptr(scores), _stream()), "fwd")
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    ds = torch.empty_like(scores)
    _lib.check(lib().nrms_ce_loss_fwd_bwd(B, Cn, _lib.ptr(scores), _lib.ptr(loss), _lib.ptr(ds), C.c_float(gs), _stream()), "ce")
    dcand, duser = torch.empty(M, d, dtype=torch.float32, device="cuda"), torch.empty(B, d, dtype=torch.float32, device="cuda")
    _lib.check(lib().nrms_click_score_bwd(B, Cn, d, _lib.ptr(cand), _lib.ptr(user), _lib.ptr(mask), _lib.ptr(ds), _lib.ptr(dcand),
                                          _lib.ptr(duser), _stream()), "bwd")
    _, allow = bounds(x, ref, gs)
    e_loss = abs(float(loss.cpu()[0]) - float(out["loss"][0]))
    e_du = np.abs(duser.cpu().numpy().astype(np.float64) - out["duser"])
    e_dc = np.abs(dcand.cpu().numpy().astype(np.float64) - out["dcand"])
    print("pooled vs row-wise B=%d C=%d d=%d masked=%d: loss %.2e of %.2e | duser %.2e | dcand %.2e"
          % (B, Cn, d, masked, e_loss, allow["loss"], float(e_du.max()), float(e_dc.max())))
    assert e_loss <= allow["loss"]
    assert (e_du <= allow["duser"]).all(), float((e_du - allow["duser"]).max())
    assert (e_dc <= allow["dcand"]).all(), float((e_dc - allow["dcand"]).max())
