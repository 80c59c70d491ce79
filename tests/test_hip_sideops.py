"""The entry points no other suite calls by name, one by one through the C ABI against tests/sideops_ref.py (float64 numpy, checked
against autograd in tests/test_sideops_ref_host.py): nrms_news_features_fwd / _bwd (csrc/wide.hip), nrms_hier_add_embedding_fwd,
nrms_hier_match, nrms_hier_query, nrms_hier_score_fwd / _bwd (csrc/hier.hip).  Whole-model parity reaches them at a few small
batches only: below 129 slots nrms_news_features_bwd never takes the chunked table-gradient path every real batch takes.

Tolerances.  Copies: np.array_equal.  One fp32 operation: the same operation in np.float32, bit for bit.  Dropout: a value times
inv_keep = fl(1 / fl(1 - p)), three roundings against v / (1 - p): 3 u |ref|.  Sums: sideops_ref.sum_bound(m, r, S[, start + ref])
= (m + r + 2) u S [+ u |start + ref|], u = 2^-24, with m (terms), r (roundings inside one term) and S (sum |term|) stated at each
use; the derivation is in tests/sideops_ref.py.  The float64 references take lambda and p as the fp32 values the library is given."""
import ctypes as C

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from tests import sideops_ref as sr
from tests.guarded import Pool

pytestmark = pytest.mark.gpu

U = sr.U
NEG = np.float32(-1e9)
SEED = 0x5EED5EED


def lib():
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def poisoned(*shape):
    """fp32 NaNs (0xFFFFFFFF): a kernel that accumulates into its output, or skips an element, shows."""
    return torch.full(shape, -1, dtype=torch.int32, device="cuda").view(torch.float32)


def within(got, ref, bound, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert np.isfinite(np.asarray(got)).all(), what
    bad = err > bound
    at = np.asarray(bound) > 0
    print("%s: largest error / bound %.3f" % (what, float((err[at] / np.asarray(bound)[at]).max(initial=0.0))))
    assert not bad.any(), "%s: %d element(s) outside the bound, worst error %.3e against %.3e at %s" % (
        what, int(bad.sum()), float(err[bad].max()), float(np.asarray(bound)[bad].min()), np.argwhere(bad)[0].tolist())


# ---- news feature rows ---------------------------------------------------------------------------------------------------------------
CASE_ID = lambda c: "n%d_dt%d_dc%d_cat%d_sub%d" % c


class Features:
    """One case's inputs on the host and on the device, drawn once per (case, seed)."""

    def __init__(self, case, seed=11, ids=None, table_dout=None):
        self.n, self.dt, self.dc, self.n_cat, self.n_sub = case
        n, dt, dc = self.n, self.dt, self.dc
        self.F = 2 * dt + 2 * dc
        rng = np.random.default_rng(seed)
        self.categ, self.sub, self.cold_cat, self.cold_sub = ids if ids is not None else sr.feature_ids(n, self.n_cat, self.n_sub, rng)
        f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
        self.title, self.abst = f32(n, dt), f32(n, dt)
        self.cat_table, self.sub_table = f32(self.n_cat, dc), f32(self.n_sub, dc)
        self.dout = f32(n, self.F)
        if table_dout is not None:
            self.dout[:, 2 * dt:] = table_dout
        self.start_cat, self.start_sub = f32(self.n_cat, dc), f32(self.n_sub, dc)       # the table gradients accumulate
        assert (self.start_cat != 0).all() and (self.start_sub != 0).all()
        self.d = {k: dev(getattr(self, k)) for k in ("title", "abst", "cat_table", "sub_table", "categ", "sub", "dout")}

    def desc(self, p):
        d = self.d
        return _lib.NewsFeatures(self.n, self.dt, self.dc, self.n_cat, self.n_sub, p, SEED, d["title"].data_ptr(), d["abst"].data_ptr(),
                                 d["cat_table"].data_ptr(), d["sub_table"].data_ptr(), d["categ"].data_ptr(), d["sub"].data_ptr())

    def keep(self, p):
        """The site-3 mask of nrms_dropout_keep_mask over [n, F].  The decisions are a function of the flat element index, and the
        export wants a width that is a multiple of 4: an odd F / 2 is replayed as [n F / 4, 4]."""
        if p == 0:
            return None
        total = self.n * self.F
        assert total % 4 == 0
        rows, width = (self.n, self.F) if self.F % 4 == 0 else (total // 4, 4)
        buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
        rc = lib().nrms_dropout_keep_mask(C.c_uint64(SEED), 3, C.c_int64(rows), width, C.c_float(p), _lib.ptr(buf), _stream())
        _lib.check(rc, "nrms_dropout_keep_mask")
        keep = host(buf).reshape(self.n, self.F)
        assert 0.1 < 1.0 - keep.mean() < 0.3 or total < 200, keep.mean()
        return keep

    def forward(self, p):
        out = poisoned(self.n, self.F)
        f = self.desc(p)
        _lib.check(lib().nrms_news_features_fwd(C.byref(f), _lib.ptr(out), _stream()), "nrms_news_features_fwd")
        return host(out)

    def backward(self, p, poison=0xFF):
        """(d_title, d_abst, d_cat_table, d_sub_table); the text gradients in guarded, poisoned buffers."""
        pool = Pool(poison)
        d_title, d_abst = pool.elems("d_title_vec", self.n * self.dt), pool.elems("d_abst_vec", self.n * self.dt)
        d_cat, d_sub = dev(self.start_cat), dev(self.start_sub)
        f = self.desc(p)
        rc = lib().nrms_news_features_bwd(C.byref(f), _lib.ptr(self.d["dout"]), d_title.ptr, d_abst.ptr, _lib.ptr(d_cat), _lib.ptr(d_sub),
                                          _stream())
        _lib.check(rc, "nrms_news_features_bwd")
        pool.intact("nrms_news_features_bwd")
        return d_title.numpy((self.n, self.dt)), d_abst.numpy((self.n, self.dt)), host(d_cat), host(d_sub)


def check_dropout(got, ref, keep, what):
    """Dropped elements exactly 0; kept ones v * inv_keep, inv_keep = fl(1 / fl(1 - p)): three roundings, 3 u |ref|."""
    assert (got[keep == 0] == 0).all(), what
    within(got, ref, 3 * U * np.abs(ref), what)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("case", sr.FEATURE_CASES, ids=CASE_ID)
def test_features_forward(case, p):
    v = Features(case)
    got = v.forward(p)
    if p == 0:
        # a gather and a concatenation: bit-equal (ids outside a table read row 0)
        fold = lambda ids, rows: np.where((ids < 0) | (ids >= rows), 0, ids)
        want = np.concatenate([v.title, v.abst, v.cat_table[fold(v.categ, v.n_cat)], v.sub_table[fold(v.sub, v.n_sub)]], axis=1)
        assert np.array_equal(bits(got), bits(want))
        return
    keep = v.keep(p)
    ref = sr.features_fwd_ref(v.title, v.abst, v.cat_table, v.sub_table, v.categ, v.sub, keep, p)
    check_dropout(got, ref, keep, "out")


def check_tables(v, g, d_cat, d_sub, r, what):
    """Row 0, the rows no slot names and every row of a table whose ids are all outside it keep their start bits; a named row
    holds start + (the sum of its m terms): sum_bound(m, r, S, start + ref), r = 0 without dropout (the terms are dout's
    elements themselves) and 3 with it (dout * inv_keep, as above)."""
    for name, got, start, cold in (("cat", d_cat, v.start_cat, v.cold_cat), ("sub", d_sub, v.start_sub, v.cold_sub)):
        m, S, ref = g["m_" + name], g["S_" + name], g["d_" + name]
        unnamed = m[:, 0] == 0
        assert unnamed[0] and unnamed[cold].all()
        assert np.array_equal(bits(got[unnamed]), bits(start[unnamed])), "%s: d_%s_table rows nobody names were written" % (what, name)
        total = start.astype(np.float64) + ref
        within(got[~unnamed], total[~unnamed], sr.sum_bound(m, r, S, total)[~unnamed], "%s: d_%s_table" % (what, name))


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("case", sr.FEATURE_CASES, ids=CASE_ID)
def test_features_backward(case, p):
    v = Features(case)
    keep = v.keep(p)
    g = sr.features_bwd_ref(v.dout, v.categ, v.sub, v.dt, v.dc, v.n_cat, v.n_sub, keep, p)
    d_title, d_abst, d_cat, d_sub = v.backward(p, 0xFF)
    # the text gradients: slices of dout through the mask.  ALL n * d_text elements of d_title_vec: the chunked path parks its
    # partial sums there and the text kernel has to overwrite every one of them
    if p == 0:
        assert np.array_equal(bits(d_title), bits(v.dout[:, :v.dt]))
        assert np.array_equal(bits(d_abst), bits(v.dout[:, v.dt:2 * v.dt]))
    else:
        check_dropout(d_title, g["d_title"], keep[:, :v.dt], "d_title_vec")
        check_dropout(d_abst, g["d_abst"], keep[:, v.dt:2 * v.dt], "d_abst_vec")
    check_tables(v, g, d_cat, d_sub, 3 if p else 0, CASE_ID(case))
    again = v.backward(p, 0x7F)                                            # no atomics: the same bits, whatever the buffers held
    for name, a, b in zip(("d_title_vec", "d_abst_vec", "d_cat_table", "d_sub_table"), (d_title, d_abst, d_cat, d_sub), again):
        assert np.array_equal(bits(a), bits(b)), name


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_features_backward_one_batch_two_paths(p):
    """The same ids and the same table columns of dout through the chunked path (d_text = 8) and through the single path
    (d_text = 1: the partial sums no longer fit into d_title_vec), both against one float64 reference.  With dropout the mask is
    indexed by n * F + c and F changes with d_text, so only p = 0 has one reference; p = 0.2 checks each path against its own."""
    n, dc, n_cat, n_sub = sr.TWO_PATH_CASE
    rng = np.random.default_rng(23)
    ids = sr.feature_ids(n, n_cat, n_sub, rng)
    table_dout = rng.standard_normal((n, 2 * dc)).astype(np.float32)
    refs = []
    for dt in sr.TWO_PATH_D_TEXT:
        v = Features((n, dt, dc, n_cat, n_sub), seed=29, ids=ids, table_dout=table_dout)
        g = sr.features_bwd_ref(v.dout, v.categ, v.sub, dt, dc, n_cat, n_sub, v.keep(p), p)
        _, _, d_cat, d_sub = v.backward(p)
        check_tables(v, g, d_cat, d_sub, 3 if p else 0, "d_text = %d" % dt)
        refs.append((g, v.start_cat, v.start_sub))
    if p == 0:                                                             # one reference indeed
        for k in ("d_cat", "d_sub", "S_cat", "S_sub", "m_cat", "m_sub"):
            assert np.array_equal(refs[0][0][k], refs[1][0][k]), k


# ---- hier_add_embedding_fwd ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots,d,n_ids", [(1, 4, 1), (65, 20, 5), (129, 300, 7), (4100, 1024, 3)])
def test_hier_add_embedding_forward(n_slots, d, n_ids):
    """u[slot] += table[id[slot]] where cnt[slot] > 0 and the id is inside the table: one fp32 addition, bit for bit; every other
    slot untouched.  4100 x 1024 floats are 1 049 600 float4s, more than the grid's 4096 x 256 lanes: the stride loop runs."""
    rng = np.random.default_rng(n_slots)
    u = rng.standard_normal((n_slots, d)).astype(np.float32)
    table = rng.standard_normal((n_ids, d)).astype(np.float32)
    ids = rng.integers(-1, n_ids + 1, n_slots).astype(np.int32)
    cnt = rng.choice([0, 3], n_slots).astype(np.int32)
    if n_slots == 1:
        ids[0], cnt[0] = 0, 3
    else:                                    # below and above the table, an empty slot with a good id, and a live last slot
        ids[:4], cnt[:4] = (-1, n_ids, 0, 0), (3, 3, 0, 3)
        ids[-1], cnt[-1] = n_ids - 1, 3
    u_d, ids_d, cnt_d, table_d = dev(u), dev(ids), dev(cnt), dev(table)
    rc = lib().nrms_hier_add_embedding_fwd(C.c_int64(n_slots), d, n_ids, _lib.ptr(ids_d), _lib.ptr(cnt_d), _lib.ptr(table_d), _lib.ptr(u_d),
                                           _stream())
    _lib.check(rc, "nrms_hier_add_embedding_fwd")
    live = (cnt > 0) & (ids >= 0) & (ids < n_ids)
    want = u.copy()
    want[live] = u[live] + table[ids[live]]                                 # np.float32 + np.float32
    assert want.dtype == np.float32 and live.any()
    got = host(u_d)
    assert np.array_equal(bits(got[~live]), bits(u[~live]))
    assert np.array_equal(bits(got), bits(want))


# ---- hier_score_fwd / _bwd -----------------------------------------------------------------------------------------------------------
LAMBDAS = [(0.7, 0.15), (0.0, 0.0)]
R_USER = 6     # roundings in one term n[k] * (cs p1[k] + ct p2[k] + lg pg[k]), longest path: lg = fl(fl(1 - l_s) - l_t) (2), lg * pg
#                (1), the two additions inside the bracket (2), the product with n[k] (1); the cs / ct paths have one fewer


def score_args(v, t):
    return (v["B"], v["C"], v["d"], _lib.ptr(t["cand"]), _lib.ptr(t["u1"]), _lib.ptr(t["u2"]), _lib.ptr(t["ug"]), _lib.ptr(t["sub_slot"]),
            _lib.ptr(t["sub_frac"]), _lib.ptr(t["top_slot"]), _lib.ptr(t["top_frac"]), _lib.ptr(t.get("mask")))


def to_dev(v):
    return {k: dev(a) for k, a in v.items() if isinstance(a, np.ndarray)}


def run_score_fwd(v, t, ls, lt):
    out = poisoned(v["B"], v["C"])
    rc = lib().nrms_hier_score_fwd(*score_args(v, t), C.c_float(ls), C.c_float(lt), _lib.ptr(out), _stream())
    _lib.check(rc, "nrms_hier_score_fwd")
    return host(out)


def check_scores(got, v, ls, lt, what):
    """m = d terms per score, r = R_USER; masked slots exactly -1e9f."""
    ref, S = sr.hier_score_ref(v["cand"], v["u1"], v["u2"], v["ug"], v["sub_slot"], v["sub_frac"], v["top_slot"], v["top_frac"], v["mask"],
                               ls, lt)
    live = np.ones(ref.shape, bool) if v["mask"] is None else v["mask"] != 0
    within(got[live], ref[live], sr.sum_bound(v["d"], R_USER, S)[live], what)
    assert (bits(got[~live]) == bits(NEG)).all(), what


SCORE_SHAPES = [(B, Cn) for B in (1, 3, 4, 5, 9) for Cn in (1, 5, 7)]


@pytest.mark.parametrize("B,Cn", SCORE_SHAPES)
@pytest.mark.parametrize("d", [1, 63, 64, 65, 300, 1024])
def test_hier_score_forward_and_backward(d, B, Cn):
    """One wave per (user, candidate) forward, one wave per user backward, 4 waves a block, lanes stride d by 64.

    Backward bounds.  dcand (overwritten): m = 3 terms ds * (c * u), r = 4 (lg: 2, lg * pg: 1, the product with ds: 1; the
    additions are the sum's).  dug (overwritten, built up from 0): m = C terms lg * (ds * n[k]), r = 4.  du1 / du2 (accumulated):
    m = the candidates that point at the row, terms cs * (ds * n[k]) with cs = fl(l_s f_s): r = 3, on top of the start value.
    The kernel adds a row's terms to the start value one candidate at a time, so the start value meets up to m rounded additions
    and not the single one u |start + ref| pays for.  The difference is at most (m - 1) u |start|, and the bound's slack over the
    m + 2 roundings a term really meets is 3 u S; the start values are therefore drawn with |start| <= 0.004, below the smallest
    non-zero term the batch can hold (0.0046, sideops_ref.hier_score_batch; zero terms round nothing), so that
    (m - 1) |start| <= 3 S whenever a rounding happens and the bound holds for the kernel's order as for any other."""
    rng = np.random.default_rng(100000 * d + 100 * B + Cn)
    for with_mask in (True, False):
        v = sr.hier_score_batch(B, Cn, d, rng, with_mask)
        t = to_dev(v)
        H = v["H"]
        start1 = (rng.uniform(0.001, 0.004, (B * H, d)) * rng.choice([-1.0, 1.0], (B * H, d))).astype(np.float32)
        start2 = (rng.uniform(0.001, 0.004, (B * H, d)) * rng.choice([-1.0, 1.0], (B * H, d))).astype(np.float32)
        for ls, lt in LAMBDAS:
            what = "mask=%s lambdas=(%g, %g)" % (with_mask, ls, lt)
            check_scores(run_score_fwd(v, t, ls, lt), v, ls, lt, what)
            runs = []
            for _ in range(2):
                dcand, dug, du1, du2 = poisoned(B, Cn, d), poisoned(B, d), dev(start1), dev(start2)
                rc = lib().nrms_hier_score_bwd(*score_args(v, t), C.c_float(ls), C.c_float(lt), _lib.ptr(t["dscores"]), _lib.ptr(dcand),
                                               _lib.ptr(du1), _lib.ptr(du2), _lib.ptr(dug), _stream())
                _lib.check(rc, "nrms_hier_score_bwd")
                runs.append([host(x) for x in (dcand, dug, du1, du2)])
            for a, b in zip(*runs):
                assert np.array_equal(bits(a), bits(b)), what                 # no atomics: two runs, the same bits
            dcand, dug, du1, du2 = runs[0]
            g = sr.hier_score_bwd_ref(v["cand"], v["u1"], v["u2"], v["ug"], v["sub_slot"], v["sub_frac"], v["top_slot"], v["top_frac"],
                                      v["mask"], ls, lt, v["dscores"])
            within(dcand, g["dcand"], sr.sum_bound(3, 4, g["S_dcand"]), what + " dcand")
            if v["mask"] is not None:
                assert (dcand[v["mask"] == 0] == 0).all(), what                 # a masked slot passes no gradient: exact zeros
            within(dug, g["dug"], sr.sum_bound(Cn, 4, g["S_dug"]), what + " dug")
            for name, got, start in (("du1", du1, start1), ("du2", du2, start2)):
                m, S = g["m_" + name], g["S_" + name]
                idle = m[:, 0] == 0
                assert idle.any()
                assert np.array_equal(bits(got[idle]), bits(start[idle])), what + " " + name       # rows nobody points at
                total = start.astype(np.float64) + g[name]
                within(got, total, sr.sum_bound(m, 3, S, total), what + " " + name)
            if (ls, lt) == (0.0, 0.0):                                         # no share of the sub-topic and topic interests
                assert np.array_equal(bits(du1), bits(start1)) and np.array_equal(bits(du2), bits(start2)), what


# ---- hier_match / hier_query ---------------------------------------------------------------------------------------------------------
GROUP_TOPIC = [sr.ID_X, sr.ID_Y, sr.ID_Z, sr.ID_X, sr.ID_Z]
GROUP_SUB = [sr.ID_X, sr.ID_Y, sr.ID_Z, sr.ID_Z, sr.ID_Y]


def run_match(B, Cn, H, cand_topic, cand_sub, lists):
    ss, ts = torch.full((B, Cn), -7, dtype=torch.int32, device="cuda"), torch.full((B, Cn), -7, dtype=torch.int32, device="cuda")
    sf, tf = poisoned(B, Cn), poisoned(B, Cn)
    topic_d, sub_d = dev(np.asarray(cand_topic, np.int64)), dev(np.asarray(cand_sub, np.int64))
    rc = lib().nrms_hier_match(B, Cn, H, _lib.ptr(topic_d), _lib.ptr(sub_d),
                               _lib.ptr(lists["l1_sub"]), _lib.ptr(lists["l1_cnt"]), _lib.ptr(lists["l2_top"]), _lib.ptr(lists["l2_cnt"]),
                               _lib.ptr(lists["n_valid"]), _lib.ptr(ss), _lib.ptr(sf), _lib.ptr(ts), _lib.ptr(tf), _stream())
    _lib.check(rc, "nrms_hier_match")
    return ss, sf, ts, tf


@pytest.mark.parametrize("H", [1, 64])
def test_hier_match_on_hand_built_lists(H):
    """Slots and shares equal hier_match_ref exactly: the share is cnt * (1 / n_valid), two fp32 operations restated in np.float32.
    What the lists hold (a user without clicks, count-0 slots carrying the id below the occupied one, two occupied slots with one
    id) is asserted on the reference in tests/test_sideops_ref_host.py."""
    v = sr.match_lists(H, np.random.default_rng(2))
    B, Cn = 4, 3
    ids = np.tile(np.asarray([sr.ID_X, sr.ID_Y, sr.ID_Z]), (B, 1))
    want = sr.hier_match_ref(B, Cn, H, ids, ids, v["l1_sub"], v["l1_cnt"], v["l2_top"], v["l2_cnt"], v["n_valid"])
    got = [host(x) for x in run_match(B, Cn, H, ids, ids, to_dev(v))]
    for name, g, w in zip(("sub_slot", "sub_frac", "top_slot", "top_frac"), got, want):
        assert g.dtype == w.dtype, name
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, g, w)
    assert (want[0][1:] >= 0).any() and (want[0] == -1).any()


@pytest.mark.parametrize("H", [1, 64])
@pytest.mark.parametrize("d,offset", [(300, 0), (63, 0), (300, 1)], ids=["d300_vector", "d63_scalar", "d300_unaligned_scalar"])
def test_hier_query(d, offset, H):
    """query[b, g] = cs u1[ss] + ct u2[ts] + lg ug[b] element-wise: m = 3 terms, r = 3 (lg: 2 and its product; cs = fl(l_s f_s) and
    its product: 2; the shares are hier_match_ref's fp32 values, exact inputs): (3 + 3 + 2) u S = 8 u S.  Then <n, query[b, g]>
    in float64 against nrms_hier_score_fwd on the slots nrms_hier_match finds for a candidate with the group's ids, within the
    forward's bound (m = d, r = R_USER).  offset: the query pointer moved by that many floats off its 16-byte alignment."""
    rng = np.random.default_rng(1000 * d + H + offset)
    v = sr.match_lists(H, rng)
    B, G = 4, len(GROUP_TOPIC)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    u1, u2, ug, cand = f32(B * H, d), f32(B * H, d), f32(B, d), f32(B, G, d)
    lists = to_dev(v)
    u1_d, u2_d, ug_d = dev(u1), dev(u2), dev(ug)
    gt_d, gs_d = dev(np.asarray(GROUP_TOPIC, np.int64)), dev(np.asarray(GROUP_SUB, np.int64))
    for ls, lt in LAMBDAS:
        buf = poisoned(B * G * d + 4)
        q_d = buf[offset:offset + B * G * d]
        assert q_d.data_ptr() % 16 == 4 * offset
        rc = lib().nrms_hier_query(B, H, G, d, _lib.ptr(gt_d), _lib.ptr(gs_d), _lib.ptr(lists["l1_sub"]), _lib.ptr(lists["l1_cnt"]), _lib.ptr(lists["l2_top"]), _lib.ptr(lists["l2_cnt"]),
                                   _lib.ptr(lists["n_valid"]), _lib.ptr(u1_d), _lib.ptr(u2_d), _lib.ptr(ug_d), C.c_float(ls), C.c_float(lt),
                                   _lib.ptr(q_d), _stream())
        _lib.check(rc, "nrms_hier_query")
        whole = host(buf)
        q = whole[offset:offset + B * G * d].reshape(B, G, d)
        outside = np.concatenate([whole[:offset], whole[offset + B * G * d:]])
        assert (outside.view(np.uint32) == 0xFFFFFFFF).all()                 # nothing written around the rows
        ref, S = sr.hier_query_ref(B, H, GROUP_TOPIC, GROUP_SUB, v["l1_sub"], v["l1_cnt"], v["l2_top"], v["l2_cnt"], v["n_valid"], u1, u2, ug,
                                   ls, lt)
        within(q, ref, 8 * U * S, "query lambdas=(%g, %g)" % (ls, lt))
        # the same users and groups as candidates of nrms_hier_score_fwd
        gt, gs = np.tile(GROUP_TOPIC, (B, 1)), np.tile(GROUP_SUB, (B, 1))
        ss, sf, ts, tf = run_match(B, G, H, gt, gs, lists)
        sv = dict(B=B, C=G, d=d, cand=cand, u1=u1, u2=u2, ug=ug, sub_slot=host(ss), sub_frac=host(sf), top_slot=host(ts), top_frac=host(tf),
                  mask=None)
        t = dict(cand=dev(cand), u1=u1_d, u2=u2_d, ug=ug_d, sub_slot=ss, sub_frac=sf, top_slot=ts, top_frac=tf)
        scores = run_score_fwd(sv, t, ls, lt)
        check_scores(scores, sv, ls, lt, "scores on matched slots")
        _, S_score = sr.hier_score_ref(cand, u1, u2, ug, sv["sub_slot"], sv["sub_frac"], sv["top_slot"], sv["top_frac"], None, ls, lt)
        dot = (q.astype(np.float64) * cand.astype(np.float64)).sum(-1)
        within(scores, dot, sr.sum_bound(d, R_USER, S_score), "query . n against hier_score_fwd")
